"""ctypes binding of libgkm.so (include/gkm.h) -- the only way this package reaches the GPU.

There is no CPU fallback: if the library is missing or no HIP device is visible, every call that
needs the engine raises.  ``Engine`` owns one ``gk_ctx`` (one device, one stream, device buffers).
"""

import ctypes
import os
from pathlib import Path

import numpy as np

GK_OK = 0
GK_E_ARG = -1
GK_E_HIP = -2
GK_E_OOM = -3
GK_E_UNSUPPORTED = -4
GK_E_ALPHABET = -5
GK_E_STATE = -6
GK_E_FILTER = -7
GK_E_LIMIT = -8
GK_E_NO_BASES = -9
GK_E_IO = -10
GK_E_FASTA_NAME = -11
GK_E_FASTA_LAYOUT = -12

# gk_filter_kind
FILTER_KEEP_ALL = 0
FILTER_LENGTH = 1
FILTER_HOMOPOLYMER = 2
FILTER_GC = 3
FILTER_NO_AMBIGUOUS = 4
FILTER_CRISPR_NGG = 5
FILTER_MASK = 6

# gk_filter_error
FERR_HOMO_LEN = 1
FERR_GC_LEN = 2
FERR_GC_OOB = 3
FERR_AMBIG_LEN = 4
FERR_AMBIG_SEG = 5
FERR_CRISPR_LEN = 6

LIB_PATH = Path(__file__).with_name("libgkm.so")
# tuning only: GKM_LIB names another build of the same library (A/B of compile-time variants)
if os.environ.get("GKM_LIB"):
    LIB_PATH = Path(os.environ["GKM_LIB"]).resolve()

# every symbol include/gkm.h declares (checked by tests/test_native_abi.py)
EXPORTED = (
    "gk_create", "gk_destroy", "gk_last_error", "gk_sync", "gk_device_count", "gk_set_sequence",
    "gk_alphabet_is_acgt", "gk_enumerate", "gk_set_start_indices", "gk_sort", "gk_num_kmers",
    "gk_copy_start_indices", "gk_copy_start_range", "gk_key_layout", "gk_copy_keys", "gk_set_filter_mask",
    "gk_set_group_heads", "gk_group_hist", "gk_group_members", "gk_unique_counts", "gk_copy_unique", "gk_device_unique", "gk_device_views",
    "gk_profile_enable", "gk_profile_report", "gk_stream", "gk_shard_bucket_bits", "gk_shard_partition",
    "gk_shard_sort", "gk_fasta_open", "gk_fasta_fill", "gk_fasta_close", "gk_locate", "gk_copy_strands",
    "gk_shard_histogram", "gk_shard_sort_range", "gk_shard_class_b", "gk_shard_class_b_copy",
    "gk_shard_sort_range_b", "gk_rank_mode", "gk_reference_random_bases",
    "gk_copy_sequence", "gk_sort_hint", "gk_resident_packed", "gk_set_option",
    "gk_lookup", "gk_copy_strand_range", "gk_lookup_mismatch",
    "gk_join", "gk_copy_join", "gk_device_join", "gk_join_mask",
    "gk_screen",
    "gk_lcp", "gk_copy_lcp", "gk_device_lcp", "gk_lcp_spectrum", "gk_position_track", "gk_device_track",
    "gk_match",
    "gk_minimizers", "gk_copy_minimizers", "gk_device_minimizers", "gk_select_minimizers",
)

SORT_CANONICAL = 1  # GK_SORT_CANONICAL
SORT_QUICKSORT_ORDER = 2  # GK_SORT_QUICKSORT_ORDER
SHARD_STARTS_ONLY = 4  # GK_SHARD_STARTS_ONLY
MISMATCH_BOTH_STRANDS = 1  # GK_MISMATCH_BOTH_STRANDS
JOIN_KEEP_ABSENT = 1  # GK_JOIN_KEEP_ABSENT
JOIN_KEEP_PRESENT = 2  # GK_JOIN_KEEP_PRESENT
SCREEN_BOTH_STRANDS = 1  # GK_SCREEN_BOTH_STRANDS
MINIMIZER_CANONICAL = 1  # GK_MINIMIZER_CANONICAL
MINIMIZER_LEX = 2  # GK_MINIMIZER_LEX
NEVER_UNIQUE = 0xFFFFFFFF  # GK_NEVER_UNIQUE
TRACK_MIN_UNIQUE = 1  # GK_TRACK_MIN_UNIQUE
TRACK_MULTIPLICITY = 2  # GK_TRACK_MULTIPLICITY


class GkFilter(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("pad", ctypes.c_int32), ("p0", ctypes.c_int64),
                ("p1", ctypes.c_int64), ("p2", ctypes.c_int64)]


class GkJoinStats(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint64) for name in ("n_distinct_a", "n_distinct_b", "n_shared", "occ_a_shared",
                                                     "occ_b_shared", "occ_min")]


class GkError(RuntimeError):
    """A libgkm call failed; ``code`` is the gk_status."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"libgkm error {code}: {msg}")
        self.code = code
        self.msg = msg


class FilterRaised(GkError):
    """A built-in filter raised on the device; carries the reference's error site."""

    def __init__(self, ferr: int, sba_idx: int):
        super().__init__(GK_E_FILTER, f"filter error {ferr} at sba index {sba_idx}")
        self.ferr = ferr
        self.sba_idx = sba_idx


_lib = None

_P = ctypes.c_void_p
_U32P = ctypes.POINTER(ctypes.c_uint32)
_U64P = ctypes.POINTER(ctypes.c_uint64)
_I64P = ctypes.POINTER(ctypes.c_int64)
_I32P = ctypes.POINTER(ctypes.c_int32)
_U8P = ctypes.POINTER(ctypes.c_uint8)

_SIGS = {
    "gk_create": ([ctypes.POINTER(_P), ctypes.c_int], ctypes.c_int),
    "gk_destroy": ([_P], None),
    "gk_last_error": ([_P], ctypes.c_char_p),
    "gk_sync": ([_P], ctypes.c_int),
    "gk_device_count": ([ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
    "gk_set_sequence": ([_P, _U8P, ctypes.c_uint64, _U32P, ctypes.c_uint64], ctypes.c_int),
    "gk_sort_hint": ([_P, ctypes.c_uint32, ctypes.c_uint32], ctypes.c_int),
    "gk_alphabet_is_acgt": ([_P, ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
    "gk_enumerate": ([_P, ctypes.c_uint32, _U64P], ctypes.c_int),
    "gk_set_start_indices": ([_P, _U32P, ctypes.c_uint64, ctypes.c_uint32], ctypes.c_int),
    "gk_sort": ([_P, ctypes.c_uint32, ctypes.c_uint32], ctypes.c_int),
    "gk_num_kmers": ([_P, _U64P], ctypes.c_int),
    "gk_copy_start_indices": ([_P, _U32P, ctypes.c_uint64], ctypes.c_int),
    "gk_copy_start_range": ([_P, ctypes.c_uint64, _U32P, ctypes.c_uint64], ctypes.c_int),
    "gk_key_layout": ([_P, _U32P, _U32P, _U32P], ctypes.c_int),
    "gk_copy_keys": ([_P, _U64P, ctypes.c_uint64], ctypes.c_int),
    "gk_set_filter_mask": ([_P, _U8P, ctypes.c_uint64], ctypes.c_int),
    "gk_set_group_heads": ([_P, _U8P, ctypes.c_uint64], ctypes.c_int),
    "gk_group_hist": ([_P, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(GkFilter), ctypes.c_int64, ctypes.c_int64,
                       ctypes.c_int64, _I64P, _I64P, _I32P, _U64P], ctypes.c_int),
    "gk_group_members": ([_P, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(GkFilter), ctypes.c_int64,
                          ctypes.c_int64, ctypes.c_int64, _U64P, _U32P, _U32P, ctypes.c_uint64, _U64P, _I32P,
                          _U64P], ctypes.c_int),
    "gk_unique_counts": ([_P, _U64P], ctypes.c_int),
    "gk_copy_unique": ([_P, _U64P, _U32P, ctypes.c_uint64], ctypes.c_int),
    "gk_device_unique": ([_P, ctypes.POINTER(_P), ctypes.POINTER(_P), _U64P], ctypes.c_int),
    "gk_device_views": ([_P, ctypes.POINTER(_P), ctypes.POINTER(_P), _U64P, _U32P], ctypes.c_int),
    "gk_profile_enable": ([_P, ctypes.c_int], ctypes.c_int),
    "gk_profile_report": ([_P, ctypes.c_char_p, ctypes.c_uint64], ctypes.c_int),
    "gk_stream": ([_P, ctypes.POINTER(_P)], ctypes.c_int),
    "gk_shard_bucket_bits": ([], ctypes.c_int),
    "gk_shard_partition": ([_P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _P, _P,
                            ctypes.c_uint64, _U64P, _U64P], ctypes.c_int),
    "gk_shard_sort": ([_P, _P, _P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _U64P, _U64P, _U32P,
                       ctypes.c_uint32], ctypes.c_int),
    "gk_shard_histogram": ([_P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _U64P, _U32P],
                           ctypes.c_int),
    "gk_shard_sort_range": ([_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _U64P],
                            ctypes.c_int),
    "gk_shard_class_b": ([_P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _U64P, _U64P,
                          _U64P], ctypes.c_int),
    "gk_shard_class_b_copy": ([_P, _U32P, ctypes.c_uint64, _U32P, ctypes.c_uint64], ctypes.c_int),
    "gk_shard_sort_range_b": ([_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _U32P,
                               ctypes.c_uint64, _U32P, ctypes.c_uint64, _U64P], ctypes.c_int),
    "gk_fasta_open": ([ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(_P), _U64P, _U64P, _U64P], ctypes.c_int),
    "gk_fasta_fill": ([_P, _U8P, ctypes.c_uint64, _U32P, ctypes.c_char_p, _U8P], ctypes.c_int),
    "gk_fasta_close": ([_P], None),
    "gk_locate": ([_P, _U64P, ctypes.c_uint64, _U32P, _U32P], ctypes.c_int),
    "gk_copy_strands": ([_P, _U8P, ctypes.c_uint64], ctypes.c_int),
    "gk_rank_mode": ([_P, ctypes.c_int, ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
    "gk_reference_random_bases": ([_U8P, ctypes.c_uint64, ctypes.c_uint32], ctypes.c_int),
    "gk_copy_sequence": ([_P, _U8P, ctypes.c_uint64], ctypes.c_int),
    "gk_resident_packed": ([_P, ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
    "gk_set_option": ([ctypes.c_char_p, ctypes.c_char_p], ctypes.c_int),
    "gk_lookup": ([_P, _U8P, ctypes.c_uint64, ctypes.c_uint32, _U64P, _U32P], ctypes.c_int),
    "gk_lookup_mismatch": ([_P, _U8P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _U64P, _U32P,
                            _U64P, _U8P, _U8P, ctypes.c_uint64, _U64P], ctypes.c_int),
    "gk_copy_strand_range": ([_P, ctypes.c_uint64, _U8P, ctypes.c_uint64], ctypes.c_int),
    "gk_join": ([_P, _P, ctypes.c_uint32, ctypes.POINTER(GkJoinStats)], ctypes.c_int),
    "gk_copy_join": ([_P, _U64P, _U32P, ctypes.c_uint64], ctypes.c_int),
    "gk_device_join": ([_P, ctypes.POINTER(_P), ctypes.POINTER(_P), _U64P], ctypes.c_int),
    "gk_join_mask": ([_P, ctypes.c_int], ctypes.c_int),
    "gk_screen": ([_P, _U8P, _U64P, ctypes.c_uint64, ctypes.c_uint32, _U32P, _U64P, _U32P], ctypes.c_int),
    "gk_match": ([_P, _U8P, _U64P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _U32P, _U32P, _U64P, _U32P,
                  _U64P, _U32P], ctypes.c_int),
    "gk_lcp": ([_P, ctypes.c_uint32, _U64P], ctypes.c_int),
    "gk_copy_lcp": ([_P, ctypes.c_uint64, _U32P, ctypes.c_uint64], ctypes.c_int),
    "gk_device_lcp": ([_P, ctypes.POINTER(_P), _U64P], ctypes.c_int),
    "gk_lcp_spectrum": ([_P, ctypes.c_uint32, _U64P, _U64P], ctypes.c_int),
    "gk_position_track": ([_P, ctypes.c_int, ctypes.c_uint32, _U32P, ctypes.c_uint64], ctypes.c_int),
    "gk_device_track": ([_P, ctypes.POINTER(_P), _U64P], ctypes.c_int),
    "gk_minimizers": ([_P, _U8P, _U64P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _U64P,
                       _U32P], ctypes.c_int),
    "gk_copy_minimizers": ([_P, _U64P, _U64P, _U8P, ctypes.c_uint64], ctypes.c_int),
    "gk_device_minimizers": ([_P, ctypes.POINTER(_P), ctypes.POINTER(_P), ctypes.POINTER(_P), _U64P], ctypes.c_int),
    "gk_select_minimizers": ([_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _U64P], ctypes.c_int),
}


def _share_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64 (soname
    libamdhip64.so.7, loaded by torch as "libamdhip64.so"); libgkm needs libamdhip64.so.7.  If
    libgkm loaded /opt/rocm's copy first, torch would later load a second runtime and fail to see
    the GPU ("No HIP GPUs are available").  Loading torch's copy first (global, without importing
    torch) makes both bind the same runtime, whichever is imported first."""
    import importlib.util

    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    for root in spec.submodule_search_locations:
        hip = Path(root) / "lib" / "libamdhip64.so"
        if hip.exists():
            ctypes.CDLL(str(hip), mode=ctypes.RTLD_GLOBAL)
            return


GROUPS_FROM_HEADS = 2  # gk_group_hist / gk_group_members: groups from gk_set_group_heads


def _group_mode(is_sorted) -> int:
    return GROUPS_FROM_HEADS if is_sorted == GROUPS_FROM_HEADS else int(bool(is_sorted))


def load_library(path: Path = LIB_PATH) -> ctypes.CDLL:
    """Load libgkm.so (raises if it has not been built -- there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not path.exists():
        raise RuntimeError(
            f"libgkm.so not found at {path}; build it with `make -C genome-kmers_amd/csrc` "
            "(genome_kmers has no CPU fallback)"
        )
    _share_hip_runtime()
    lib = ctypes.CDLL(str(path))
    for name, (args, res) in _SIGS.items():
        if os.environ.get("GKM_LIB") and not hasattr(lib, name):
            continue  # an older build under A/B (tuning only): entry points it lacks stay unbound
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


class FastaLayoutError(Exception):
    """gk_fasta_fill found bytes that would not fill the sba exactly (the reference asserts)."""


def read_fasta(path, n_threads: int = 0):
    """FASTA -> (sba uint8, seg_starts uint32, names list[str], bad byte values) with libgkm's
    multithreaded host parser (gk_fasta_open / gk_fasta_fill); the caller applies the reference's
    checks.  The sba length is total_seq_len + num_records - 1, allocated exactly as
    sequence_collection.py:531-533 does (so an empty file fails the same way)."""
    lib = load_library()
    with open(path, "rb"):  # the reference's open(): FileNotFoundError etc. with its messages
        pass
    h = _P()
    nrec, total, nbytes = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib.gk_fasta_open(str(path).encode(), int(n_threads), ctypes.byref(h), ctypes.byref(nrec),
                           ctypes.byref(total), ctypes.byref(nbytes))
    if rc != GK_OK:
        raise OSError(f"cannot map {path} (libgkm error {rc})")
    try:
        sba_len = int(total.value) + int(nrec.value) - 1
        sba = np.zeros(sba_len, dtype=np.uint8)
        seg_starts = np.zeros(int(nrec.value), dtype=np.uint32)
        names = ctypes.create_string_buffer(max(int(nbytes.value), 1))
        bad = np.zeros(256, dtype=np.uint8)
        rc = lib.gk_fasta_fill(h, _ptr(sba, ctypes.c_uint8), sba_len, _ptr(seg_starts, ctypes.c_uint32), names,
                               _ptr(bad, ctypes.c_uint8))
    finally:
        lib.gk_fasta_close(h)
    if rc == GK_E_FASTA_NAME:
        raise IndexError("list index out of range")  # line[1:].strip().split()[0] on an empty name
    if rc == GK_E_FASTA_LAYOUT:
        raise FastaLayoutError()
    if rc != GK_OK:
        raise GkError(rc, "gk_fasta_fill failed")
    raw = names.raw[: int(nbytes.value)]
    name_list = [b.decode("utf-8") for b in raw.split(b"\0")[:-1]] if nrec.value else []
    return sba, seg_starts, name_list, set(np.flatnonzero(bad).tolist())


def reference_random_bases(n: int, seed: int) -> np.ndarray:
    """The reference's profiling genome (profiling.get_random_seq after np.random.seed(seed)) as n
    ASCII bytes, from libgkm's host MT19937 (gk_reference_random_bases)."""
    out = np.empty(n, dtype=np.uint8)
    lib = load_library()
    if os.environ.get("GKM_LIB") and not hasattr(lib, "gk_reference_random_bases"):
        # an older build under A/B (tuning only): the in-tree library's generator
        lib = ctypes.CDLL(str(Path(__file__).with_name("libgkm.so")))
        lib.gk_reference_random_bases.argtypes = _SIGS["gk_reference_random_bases"][0]
    rc = lib.gk_reference_random_bases(_ptr(out, ctypes.c_uint8), n, int(seed) & 0xFFFFFFFF)
    if rc != GK_OK:
        raise GkError(rc, "gk_reference_random_bases failed")
    return out


class _Options(dict):
    """libgkm's test and tuning overrides (gk_set_option), as a dict: ``options["GKM_X"] = "1"`` sets
    one, ``del options["GKM_X"]`` clears it -- so pytest's ``monkeypatch.setitem(options, ...)``
    restores the library state after a test.  Process-wide; names start with GKM_."""

    def __setitem__(self, name, value):
        rc = load_library().gk_set_option(name.encode(), str(value).encode())
        if rc != GK_OK:
            raise GkError(rc, f"gk_set_option({name!r}) failed")
        super().__setitem__(name, str(value))

    def __delitem__(self, name):
        super().__delitem__(name)  # (KeyError if unset, as a dict)
        load_library().gk_set_option(name.encode(), None)


options = _Options()


def _ptr(arr: np.ndarray, ctype):
    return arr.ctypes.data_as(ctypes.POINTER(ctype))


QUERY_ALPHABET = b"ABCDGHKMNRSTVWY"  # the sba alphabet without '$' (gk_lookup's query bytes)
_QUERY_OK = np.zeros(256, dtype=bool)
_QUERY_OK[np.frombuffer(QUERY_ALPHABET, dtype=np.uint8)] = True


def pack_queries(kmers, kmer_len: int = None) -> np.ndarray:
    """The query batch of gk_lookup: a C-contiguous uint8 array [m, q] of ASCII bytes.  Host only.

    ``kmers``: one ``str`` / ``bytes`` (m = 1), a sequence of them (all of one length), or a 2-D uint8
    array.  ValueError: ragged lengths, an empty k-mer, a character outside ABCDGHKMNRSTVWY (upper
    case; the message names the query's index and the character), or ``kmer_len`` given and different
    from the k-mers' length."""
    if isinstance(kmers, np.ndarray):
        if kmers.ndim != 2 or kmers.dtype != np.uint8:
            raise ValueError(f"a query array must be 2-D uint8 (ndim = {kmers.ndim}, dtype = {kmers.dtype})")
        arr = np.ascontiguousarray(kmers)
        if arr.shape[0] > 0 and arr.shape[1] == 0:
            raise ValueError("k-mer 0 is empty")
    else:
        if isinstance(kmers, (str, bytes, bytearray)):
            kmers = [kmers]
        rows = []
        for i, k in enumerate(kmers):
            if isinstance(k, str):
                try:
                    k = k.encode("ascii")
                except UnicodeEncodeError:
                    bad = next(ch for ch in k if ord(ch) > 127)
                    raise ValueError(f"k-mer {i} holds the character {bad!r}, outside the alphabet "
                                     f"{QUERY_ALPHABET.decode()}") from None
            elif not isinstance(k, (bytes, bytearray)):
                raise ValueError(f"k-mer {i} is neither str nor bytes ({type(k).__name__})")
            if len(k) == 0:
                raise ValueError(f"k-mer {i} is empty")
            if rows and len(k) != len(rows[0]):
                raise ValueError(f"k-mers differ in length: k-mer {i} has {len(k)} characters, k-mer 0 has "
                                 f"{len(rows[0])}")
            rows.append(bytes(k))
        q = len(rows[0]) if rows else (int(kmer_len) if kmer_len else 1)
        arr = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), q)
    if kmer_len is not None and arr.shape[0] > 0 and arr.shape[1] != kmer_len:
        raise ValueError(f"the k-mers have {arr.shape[1]} characters, kmer_len is {kmer_len}")
    ok = _QUERY_OK[arr]
    if not ok.all():
        i, j = np.argwhere(~ok)[0]
        raise ValueError(f"k-mer {int(i)} holds the character {chr(int(arr[i, j]))!r}, outside the alphabet "
                         f"{QUERY_ALPHABET.decode()}")
    return arr


def pack_sequences(seqs):
    """The read batch of gk_screen: ``(uint8[total], uint64[nseq + 1])``, the sequences' ASCII bytes
    back to back and their offsets (sequence j is ``[offsets[j], offsets[j + 1])``).  Host only.

    ``seqs``: one ``str`` / ``bytes`` (a batch of one), a list of them (any lengths, empty ones
    allowed), or an already packed ``(array, offsets)`` pair, whose offsets must start at 0, never
    decrease and end at the array's length.  ValueError: such offsets, an entry that is neither str nor
    bytes, a character outside ABCDGHKMNRSTVWY (upper case; the message names the sequence's index,
    the offset in it and the character)."""
    if isinstance(seqs, (str, bytes, bytearray)):
        seqs = [seqs]
    if isinstance(seqs, tuple) and len(seqs) == 2 and isinstance(seqs[0], np.ndarray):
        arr, offsets = seqs
        if arr.ndim != 1 or arr.dtype != np.uint8:
            raise ValueError(f"a packed sequence array must be 1-D uint8 (ndim = {arr.ndim}, dtype = {arr.dtype})")
        arr = np.ascontiguousarray(arr)
        off = np.asarray(offsets)
        if off.ndim != 1 or off.size == 0 or off.dtype.kind not in "iu" or (off.dtype.kind == "i" and (off < 0).any()):
            raise ValueError("offsets must be a 1-D array of nseq + 1 non-negative integers")
        off = np.ascontiguousarray(off, dtype=np.uint64)
        if off[0] != 0 or off[-1] != arr.size or (off[1:] < off[:-1]).any():
            raise ValueError(f"offsets must start at 0, never decrease and end at the array's length ({arr.size})")
    else:
        parts = []
        for i, s in enumerate(seqs):
            if isinstance(s, str):
                try:
                    s = s.encode("ascii")
                except UnicodeEncodeError:
                    j, bad = next((j, ch) for j, ch in enumerate(s) if ord(ch) > 127)
                    raise ValueError(f"sequence {i} holds the character {bad!r} at offset {j}, outside the alphabet "
                                     f"{QUERY_ALPHABET.decode()}") from None
            elif not isinstance(s, (bytes, bytearray)):
                raise ValueError(f"sequence {i} is neither str nor bytes ({type(s).__name__})")
            parts.append(bytes(s))
        arr = np.frombuffer(b"".join(parts), dtype=np.uint8)
        off = np.zeros(len(parts) + 1, dtype=np.uint64)
        np.cumsum(np.array([len(p) for p in parts], dtype=np.uint64), out=off[1:])
    ok = _QUERY_OK[arr]
    if not ok.all():
        pos = int(np.argmin(ok))
        j = int(np.searchsorted(off, pos, side="right")) - 1
        raise ValueError(f"sequence {j} holds the character {chr(int(arr[pos]))!r} at offset {pos - int(off[j])}, "
                         f"outside the alphabet {QUERY_ALPHABET.decode()}")
    return arr, off


def device_count() -> int:
    lib = load_library()
    n = ctypes.c_int(0)
    if lib.gk_device_count(ctypes.byref(n)) != GK_OK:
        return 0
    return n.value


def default_device() -> int:
    return int(os.environ.get("GENOME_KMERS_DEVICE", os.environ.get("LOCAL_RANK", "0")))


class Engine:
    """One libgkm context: a sequence byte array resident in HBM plus its k-mer arrays."""

    def __init__(self, device: int = None):
        self.lib = load_library()
        self.device = default_device() if device is None else device
        self.ctx = _P()
        rc = self.lib.gk_create(ctypes.byref(self.ctx), self.device)
        if rc != GK_OK:
            self.ctx = None
            raise GkError(rc, f"cannot create a HIP context on device {self.device}: genome_kmers needs an "
                              "MI355X (gfx950) GPU and has no CPU fallback")
        self.n = 0

    def __del__(self):
        ctx = getattr(self, "ctx", None)
        if ctx:
            self.lib.gk_destroy(ctx)
            self.ctx = None

    def rank_mode(self, mode: int = -1) -> int:
        """Partition ranking on this engine's device (gk_rank_mode): mode -1 queries, 0 restores the
        device's checked default, 1 forces the ballot-match fallback.  Returns 1 if ballot-match
        ranking is in use afterwards."""
        active = ctypes.c_int(0)
        self._check(self.lib.gk_rank_mode(self.ctx, int(mode), ctypes.byref(active)))
        return active.value

    # -----------------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != GK_OK:
            msg = self.lib.gk_last_error(self.ctx)
            raise GkError(rc, msg.decode() if msg else "")

    def set_sequence(self, sba: np.ndarray, seg_starts: np.ndarray):
        sba = np.ascontiguousarray(sba, dtype=np.uint8)
        seg = np.ascontiguousarray(seg_starts, dtype=np.uint32)
        self._check(self.lib.gk_set_sequence(self.ctx, _ptr(sba, ctypes.c_uint8), sba.size,
                                             _ptr(seg, ctypes.c_uint32), seg.size))

    def sort_hint(self, k: int):
        """gk_sort_hint: later set_sequence calls of a single-contig A/C/G/T sequence also run the
        first pass of sort(k) while the sequence streams in (0 clears)."""
        self._check(self.lib.gk_sort_hint(self.ctx, int(k or 0), 0))

    def is_acgt(self) -> bool:
        v = ctypes.c_int(0)
        self._check(self.lib.gk_alphabet_is_acgt(self.ctx, ctypes.byref(v)))
        return bool(v.value)

    def resident_packed(self) -> bool:
        """The 2-bit packed copy of the sequence is resident (gk_resident_packed)."""
        v = ctypes.c_int(0)
        self._check(self.lib.gk_resident_packed(self.ctx, ctypes.byref(v)))
        return bool(v.value)

    def enumerate(self, min_kmer_len: int) -> int:
        n = ctypes.c_uint64(0)
        self._check(self.lib.gk_enumerate(self.ctx, min_kmer_len, ctypes.byref(n)))
        self.n = n.value
        return self.n

    def copy_sequence(self, length: int) -> np.ndarray:
        """The device-resident sba (gk_copy_sequence)."""
        out = np.empty(length, dtype=np.uint8)
        self._check(self.lib.gk_copy_sequence(self.ctx, _ptr(out, ctypes.c_uint8), length))
        return out

    def set_start_indices(self, starts: np.ndarray, min_kmer_len: int):
        arr = np.ascontiguousarray(starts, dtype=np.uint32)
        self._check(self.lib.gk_set_start_indices(self.ctx, _ptr(arr, ctypes.c_uint32), arr.size, min_kmer_len))
        self.n = arr.size

    def sort(self, max_kmer_len: int = None, canonical: bool = False, quicksort_order: bool = False):
        flags = (SORT_CANONICAL if canonical else 0) | (SORT_QUICKSORT_ORDER if quicksort_order else 0)
        self._check(self.lib.gk_sort(self.ctx, 0 if max_kmer_len is None else int(max_kmer_len), flags))

    def copy_strands(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.uint8)
        self._check(self.lib.gk_copy_strands(self.ctx, _ptr(out, ctypes.c_uint8), out.size))
        return out

    def sync(self):
        self._check(self.lib.gk_sync(self.ctx))

    def copy_starts(self, out: np.ndarray = None) -> np.ndarray:
        if out is None:
            out = np.empty(self.n, dtype=np.uint32)
        self._check(self.lib.gk_copy_start_indices(self.ctx, _ptr(out, ctypes.c_uint32), self.n))
        return out

    def start_range(self, offset: int, count: int) -> np.ndarray:
        out = np.empty(count, dtype=np.uint32)
        self._check(self.lib.gk_copy_start_range(self.ctx, offset, _ptr(out, ctypes.c_uint32), count))
        return out

    def key_layout(self):
        w, b, s = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self.lib.gk_key_layout(self.ctx, ctypes.byref(w), ctypes.byref(b), ctypes.byref(s)))
        return w.value, b.value, s.value

    def copy_keys(self) -> np.ndarray:
        words, _, _ = self.key_layout()
        out = np.empty((self.n, words), dtype=np.uint64)
        self._check(self.lib.gk_copy_keys(self.ctx, _ptr(out, ctypes.c_uint64), out.size))
        return out

    def set_filter_mask(self, mask: np.ndarray):
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        self._check(self.lib.gk_set_filter_mask(self.ctx, _ptr(m, ctypes.c_uint8), m.size))

    def set_group_heads(self, heads: np.ndarray):
        h = np.ascontiguousarray(heads, dtype=np.uint8)
        self._check(self.lib.gk_set_group_heads(self.ctx, _ptr(h, ctypes.c_uint8), h.size))

    def _raise_filter(self, rc, code, idx):
        if rc == GK_E_FILTER:
            raise FilterRaised(code.value, idx.value)
        self._check(rc)

    def group_hist(self, is_sorted, kmer_len, filt: GkFilter, min_group_size, max_group_size, max_counts_bin):
        hist = np.zeros(max_counts_bin + 1, dtype=np.int64)
        total = ctypes.c_int64(0)
        code, idx = ctypes.c_int32(0), ctypes.c_uint64(0)
        rc = self.lib.gk_group_hist(self.ctx, _group_mode(is_sorted), -1 if kmer_len is None else int(kmer_len),
                                    ctypes.byref(filt), int(min_group_size),
                                    -1 if max_group_size is None else int(max_group_size), int(max_counts_bin),
                                    _ptr(hist, ctypes.c_int64), ctypes.byref(total), ctypes.byref(code),
                                    ctypes.byref(idx))
        self._raise_filter(rc, code, idx)
        return hist, int(total.value)

    def group_members(self, is_sorted, kmer_len, filt: GkFilter, min_group_size, max_group_size, yield_first_n):
        args = (_group_mode(is_sorted), -1 if kmer_len is None else int(kmer_len), ctypes.byref(filt),
                int(min_group_size), -1 if max_group_size is None else int(max_group_size),
                -1 if yield_first_n is None else int(yield_first_n))
        count = ctypes.c_uint64(0)
        code, idx = ctypes.c_int32(0), ctypes.c_uint64(0)
        rc = self.lib.gk_group_members(self.ctx, *args, None, None, None, 0, ctypes.byref(count),
                                       ctypes.byref(code), ctypes.byref(idx))
        self._raise_filter(rc, code, idx)
        m = count.value
        num = np.empty(m, dtype=np.uint64)
        yld = np.empty(m, dtype=np.uint32)
        tot = np.empty(m, dtype=np.uint32)
        if m:
            rc = self.lib.gk_group_members(self.ctx, *args, _ptr(num, ctypes.c_uint64), _ptr(yld, ctypes.c_uint32),
                                           _ptr(tot, ctypes.c_uint32), m, ctypes.byref(count), ctypes.byref(code),
                                           ctypes.byref(idx))
            self._raise_filter(rc, code, idx)
        return num, yld, tot

    def unique_counts(self):
        g = ctypes.c_uint64(0)
        self._check(self.lib.gk_unique_counts(self.ctx, ctypes.byref(g)))
        starts = np.empty(g.value, dtype=np.uint64)
        counts = np.empty(g.value, dtype=np.uint32)
        self._check(self.lib.gk_copy_unique(self.ctx, _ptr(starts, ctypes.c_uint64), _ptr(counts, ctypes.c_uint32),
                                            g.value))
        return starts, counts

    def locate(self, kmer_nums: np.ndarray):
        """(start sba index, segment) of each kmer_num, on the device (gk_locate)."""
        nums = np.ascontiguousarray(kmer_nums, dtype=np.uint64)
        m = len(nums)
        sba_idx = np.empty(m, dtype=np.uint32)
        seg = np.empty(m, dtype=np.uint32)
        if m:
            self._check(self.lib.gk_locate(self.ctx, _ptr(nums, ctypes.c_uint64), m, _ptr(sba_idx, ctypes.c_uint32),
                                           _ptr(seg, ctypes.c_uint32)))
        return sba_idx, seg

    def lookup(self, queries: np.ndarray):
        """(first uint64[m], count uint32[m]) of a pack_queries batch [m, q] in the sorted order
        (gk_lookup): the matches of query j are the sorted positions [first[j], first[j] + count[j])."""
        q = np.ascontiguousarray(queries, dtype=np.uint8)
        if q.ndim != 2:
            raise ValueError(f"queries must be a 2-D uint8 array (ndim = {q.ndim})")
        m, qlen = q.shape
        first = np.empty(m, dtype=np.uint64)
        count = np.empty(m, dtype=np.uint32)
        if m:
            self._check(self.lib.gk_lookup(self.ctx, _ptr(q, ctypes.c_uint8), m, qlen, _ptr(first, ctypes.c_uint64),
                                           _ptr(count, ctypes.c_uint32)))
        return first, count

    def _mismatch_args(self, queries, max_mismatches, both_strands):
        q = np.ascontiguousarray(queries, dtype=np.uint8)
        if q.ndim != 2:
            raise ValueError(f"queries must be a 2-D uint8 array (ndim = {q.ndim})")
        if max_mismatches < 0:
            raise ValueError(f"max_mismatches ({max_mismatches}) must be >= 0")
        return q, (MISMATCH_BOTH_STRANDS if both_strands else 0)

    def mismatch_counts(self, queries: np.ndarray, max_mismatches: int, both_strands: bool = False) -> np.ndarray:
        """uint64[m, max_mismatches + 1]: for each query of a pack_queries batch [m, q] the number of
        (position of the current order, strand) pairs at each distance 0..max_mismatches
        (gk_lookup_mismatch, counts only)."""
        q, flags = self._mismatch_args(queries, max_mismatches, both_strands)
        m, qlen = q.shape
        counts = np.zeros((m, int(max_mismatches) + 1), dtype=np.uint64)
        total = ctypes.c_uint64(0)
        if m:
            self._check(self.lib.gk_lookup_mismatch(self.ctx, _ptr(q, ctypes.c_uint8), m, qlen, int(max_mismatches),
                                                    flags, _ptr(counts, ctypes.c_uint64), None, None, None, None, 0,
                                                    ctypes.byref(total)))
        return counts

    def mismatch_hits(self, queries: np.ndarray, max_mismatches: int, both_strands: bool = False,
                      max_hits: int = 1 << 26):
        """(counts, query uint32[h], kmer_num uint64[h], mismatches uint8[h], strand uint8[h]): the
        hits of gk_lookup_mismatch in ascending (query, kmer_num, strand), by a counts call and then a
        hits call.  ValueError (naming the total) when there are more than max_hits."""
        q, flags = self._mismatch_args(queries, max_mismatches, both_strands)
        m, qlen = q.shape
        counts = self.mismatch_counts(q, max_mismatches, both_strands)
        h = int(counts.sum())
        if h > max_hits:
            raise ValueError(f"the search has {h} hits, more than max_hits ({max_hits})")
        query = np.empty(h, dtype=np.uint32)
        num = np.empty(h, dtype=np.uint64)
        mism = np.empty(h, dtype=np.uint8)
        strand = np.empty(h, dtype=np.uint8)
        total = ctypes.c_uint64(0)
        if h:
            self._check(self.lib.gk_lookup_mismatch(self.ctx, _ptr(q, ctypes.c_uint8), m, qlen, int(max_mismatches),
                                                    flags, _ptr(counts, ctypes.c_uint64), _ptr(query, ctypes.c_uint32),
                                                    _ptr(num, ctypes.c_uint64), _ptr(mism, ctypes.c_uint8),
                                                    _ptr(strand, ctypes.c_uint8), h, ctypes.byref(total)))
        return counts, query, num, mism, strand

    def strand_range(self, offset: int, count: int) -> np.ndarray:
        """copy_strands for the sorted positions [offset, offset + count) (gk_copy_strand_range)."""
        out = np.empty(count, dtype=np.uint8)
        self._check(self.lib.gk_copy_strand_range(self.ctx, int(offset), _ptr(out, ctypes.c_uint8), int(count)))
        return out

    # ---- two genomes (gk_join) -----------------------------------------------------------------
    def join(self, other: "Engine") -> dict:
        """Look every distinct k-mer of this engine's sorted order up in ``other``'s (gk_join); the six
        sums of gk_join_stats as a dict.  The result stays on the device (join_result, join_mask)."""
        if not isinstance(other, Engine):
            raise TypeError(f"join needs an Engine (got {type(other).__name__})")
        st = GkJoinStats()
        self._check(self.lib.gk_join(self.ctx, other.ctx, 0, ctypes.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in GkJoinStats._fields_}

    def join_result(self):
        """(b_first uint64[u], b_count uint32[u]) of the last join, aligned with unique_counts()
        (gk_device_join for the length, gk_copy_join)."""
        n = ctypes.c_uint64(0)
        self._check(self.lib.gk_device_join(self.ctx, None, None, ctypes.byref(n)))
        first = np.empty(n.value, dtype=np.uint64)
        count = np.empty(n.value, dtype=np.uint32)
        self._check(self.lib.gk_copy_join(self.ctx, _ptr(first, ctypes.c_uint64), _ptr(count, ctypes.c_uint32),
                                          n.value))
        return first, count

    def join_mask(self, keep: int):
        """The filter mask of FILTER_MASK written on the device from the last join (gk_join_mask):
        keep = JOIN_KEEP_ABSENT or JOIN_KEEP_PRESENT."""
        self._check(self.lib.gk_join_mask(self.ctx, int(keep)))

    # ---- reads against the index (gk_screen) ---------------------------------------------------
    def screen(self, seqs: np.ndarray, offsets: np.ndarray, both_strands: bool = False, per_window: bool = False):
        """(n_present uint32[nseq], occurrences uint64[nseq], window_counts uint32[total] or None) of
        a pack_sequences batch against the sorted order (gk_screen)."""
        arr = np.ascontiguousarray(seqs, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if arr.ndim != 1 or off.ndim != 1 or off.size == 0:
            raise ValueError("screen takes a 1-D uint8 array and its nseq + 1 offsets")
        nseq = off.size - 1
        n_present = np.zeros(nseq, dtype=np.uint32)
        occurrences = np.zeros(nseq, dtype=np.uint64)
        wc = np.zeros(arr.size, dtype=np.uint32) if per_window else None
        if nseq:
            self._check(self.lib.gk_screen(self.ctx, _ptr(arr, ctypes.c_uint8), _ptr(off, ctypes.c_uint64), nseq,
                                           SCREEN_BOTH_STRANDS if both_strands else 0, _ptr(n_present, ctypes.c_uint32),
                                           _ptr(occurrences, ctypes.c_uint64),
                                           _ptr(wc, ctypes.c_uint32) if per_window else None))
        return n_present, occurrences, wc

    # ---- matching statistics of reads (gk_match) ------------------------------------------------
    def match(self, seqs: np.ndarray, offsets: np.ndarray, max_len: int = 0, per_position=True):
        """(longest uint32[nseq], longest_pos uint32[nseq], sum_len uint64[nseq], lengths uint32[total],
        first uint64[total], count uint32[total]) of a pack_sequences batch against the sorted order
        (gk_match); max_len 0: the sort length.  ``per_position``: True or False for all three
        per-position arrays, or three flags (lengths, first, count); an array not asked for is None."""
        arr = np.ascontiguousarray(seqs, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if arr.ndim != 1 or off.ndim != 1 or off.size == 0:
            raise ValueError("match takes a 1-D uint8 array and its nseq + 1 offsets")
        want = (bool(per_position),) * 3 if isinstance(per_position, (bool, np.bool_)) else tuple(map(bool, per_position))
        if len(want) != 3:
            raise ValueError("per_position is a bool or three of them (lengths, first, count)")
        nseq = off.size - 1
        longest = np.zeros(nseq, dtype=np.uint32)
        longest_pos = np.zeros(nseq, dtype=np.uint32)
        sum_len = np.zeros(nseq, dtype=np.uint64)
        lengths = np.zeros(arr.size, dtype=np.uint32) if want[0] else None
        first = np.zeros(arr.size, dtype=np.uint64) if want[1] else None
        count = np.zeros(arr.size, dtype=np.uint32) if want[2] else None
        if nseq:
            self._check(self.lib.gk_match(self.ctx, _ptr(arr, ctypes.c_uint8), _ptr(off, ctypes.c_uint64), nseq,
                                          int(max_len), 0, _ptr(longest, ctypes.c_uint32),
                                          _ptr(longest_pos, ctypes.c_uint32), _ptr(sum_len, ctypes.c_uint64),
                                          _ptr(lengths, ctypes.c_uint32) if want[0] else None,
                                          _ptr(first, ctypes.c_uint64) if want[1] else None,
                                          _ptr(count, ctypes.c_uint32) if want[2] else None))
        return longest, longest_pos, sum_len, lengths, first, count

    # ---- minimizer sampling (gk_minimizers, gk_select_minimizers) -------------------------------
    def minimizers(self, packed, k: int, w: int, flags: int = 0):
        """(pos uint64[n] in the batch, key uint64[n], strand uint8[n], per_seq uint32[nseq]) of a
        pack_sequences batch (gk_minimizers, then gk_copy_minimizers of the device view)."""
        arr = np.ascontiguousarray(packed[0], dtype=np.uint8)
        off = np.ascontiguousarray(packed[1], dtype=np.uint64)
        if arr.ndim != 1 or off.ndim != 1 or off.size == 0:
            raise ValueError("minimizers takes a 1-D uint8 array and its nseq + 1 offsets")
        nseq = off.size - 1
        n = ctypes.c_uint64(0)
        per_seq = np.zeros(nseq, dtype=np.uint32)
        self._check(self.lib.gk_minimizers(self.ctx, _ptr(arr, ctypes.c_uint8), _ptr(off, ctypes.c_uint64), nseq,
                                           int(k), int(w), int(flags), ctypes.byref(n),
                                           _ptr(per_seq, ctypes.c_uint32) if nseq else None))
        pos = np.empty(n.value, dtype=np.uint64)
        key = np.empty(n.value, dtype=np.uint64)
        strand = np.empty(n.value, dtype=np.uint8)
        self._check(self.lib.gk_copy_minimizers(self.ctx, _ptr(pos, ctypes.c_uint64), _ptr(key, ctypes.c_uint64),
                                                _ptr(strand, ctypes.c_uint8), n.value))
        return pos, key, strand, per_seq

    def device_minimizers(self):
        """(pos uint64*, key uint64*, strand uint8*, n) of the last minimizers (gk_device_minimizers)."""
        p, q, s, n = _P(), _P(), _P(), ctypes.c_uint64()
        self._check(self.lib.gk_device_minimizers(self.ctx, ctypes.byref(p), ctypes.byref(q), ctypes.byref(s),
                                                  ctypes.byref(n)))
        return p.value, q.value, s.value, n.value

    def select_minimizers(self, k: int, w: int, flags: int = 0) -> int:
        """The loaded sequence's minimizers become the start set (gk_select_minimizers); their number."""
        n = ctypes.c_uint64(0)
        self._check(self.lib.gk_select_minimizers(self.ctx, int(k), int(w), int(flags), ctypes.byref(n)))
        self.n = n.value
        return self.n

    # ---- the LCP array of the sorted order (gk_lcp) -------------------------------------------
    def lcp(self, max_len: int) -> np.ndarray:
        """uint32[n]: the common prefix, at most max_len, of every sorted k-mer with its predecessor
        (gk_lcp builds or reuses the device view, gk_copy_lcp copies it clamped to max_len)."""
        n = ctypes.c_uint64(0)
        self._check(self.lib.gk_lcp(self.ctx, int(max_len), ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.uint32)
        if n.value:
            self._check(self.lib.gk_copy_lcp(self.ctx, 0, _ptr(out, ctypes.c_uint32), n.value))
        return out

    def device_lcp(self):
        """(device pointer of the view uint32*, n) of the last lcp (gk_device_lcp)."""
        p, n = _P(), ctypes.c_uint64()
        self._check(self.lib.gk_device_lcp(self.ctx, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def lcp_spectrum(self, max_len: int):
        """(distinct int64[max_len + 1], unique int64[max_len + 1]) indexed by k (gk_lcp_spectrum)."""
        distinct = np.zeros(int(max_len) + 1, dtype=np.uint64)
        unique = np.zeros(int(max_len) + 1, dtype=np.uint64)
        self._check(self.lib.gk_lcp_spectrum(self.ctx, int(max_len), _ptr(distinct, ctypes.c_uint64),
                                             _ptr(unique, ctypes.c_uint64)))
        return distinct.astype(np.int64), unique.astype(np.int64)

    def position_track(self, kind: int, length: int, sba_len: int) -> np.ndarray:
        """uint32[sba_len] in sequence order (gk_position_track): kind = TRACK_MIN_UNIQUE (length: the
        cap) or TRACK_MULTIPLICITY (length: kmer_len, 0 = the sort length)."""
        out = np.zeros(int(sba_len), dtype=np.uint32)
        self._check(self.lib.gk_position_track(self.ctx, int(kind), int(length), _ptr(out, ctypes.c_uint32),
                                               int(sba_len)))
        return out

    def device_track(self):
        """(device pointer uint32*, sba_len) of the last position track (gk_device_track)."""
        p, n = _P(), ctypes.c_uint64()
        self._check(self.lib.gk_device_track(self.ctx, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    # ---- multi-GPU shards (genome_kmers.distributed) ------------------------------------------
    def shard_bucket_bits(self) -> int:
        return int(self.lib.gk_shard_bucket_bits())

    def shard_partition(self, lo: int, hi: int, k: int, keys, starts, canonical: bool = False,
                        starts_only: bool = False):
        """Encode + partition the k-mers starting in [lo, hi) into the device tensors ``keys``
        (int64) / ``starts`` (int32); returns (bucket sizes as a numpy uint64 array, count).
        starts_only (GK_SHARD_STARTS_ONLY): ``keys`` may be None, only the starts are written."""
        hist = np.zeros(1 << self.shard_bucket_bits(), dtype=np.uint64)
        n = ctypes.c_uint64(0)
        cap = starts.numel() if keys is None else min(keys.numel(), starts.numel())
        flags = (SORT_CANONICAL if canonical else 0) | (SHARD_STARTS_ONLY if starts_only else 0)
        self._check(self.lib.gk_shard_partition(self.ctx, lo, hi, k, flags, None if keys is None else keys.data_ptr(),
                                                starts.data_ptr(), cap, _ptr(hist, ctypes.c_uint64), ctypes.byref(n)))
        return hist, n.value

    def shard_sort(self, keys, starts, n: int, k: int, piece_off: np.ndarray, piece_len: np.ndarray,
                   piece_bucket: np.ndarray, canonical: bool = False, starts_only: bool = False):
        """Sort n received (key, start) pairs held in device tensors, given as bucket pieces.
        starts_only (GK_SHARD_STARTS_ONLY): ``keys`` may be None, the keys are re-derived from the
        resident sequence."""
        off = np.ascontiguousarray(piece_off, dtype=np.uint64)
        ln = np.ascontiguousarray(piece_len, dtype=np.uint64)
        bk = np.ascontiguousarray(piece_bucket, dtype=np.uint32)
        flags = (SORT_CANONICAL if canonical else 0) | (SHARD_STARTS_ONLY if starts_only else 0)
        self._check(self.lib.gk_shard_sort(self.ctx, keys.data_ptr() if n and keys is not None else None,
                                           starts.data_ptr() if n else None, n, k, flags, _ptr(off, ctypes.c_uint64),
                                           _ptr(ln, ctypes.c_uint64), _ptr(bk, ctypes.c_uint32), len(bk)))
        self.n = n

    def shard_histogram(self, lo: int, hi: int, k: int, canonical: bool = False):
        """Top-digit histogram of the k-mers starting in [lo, hi): (numpy uint64[1 << bits], bits)."""
        hist = np.zeros(4096, dtype=np.uint64)
        bits = ctypes.c_uint32(0)
        self._check(self.lib.gk_shard_histogram(self.ctx, lo, hi, k, SORT_CANONICAL if canonical else 0,
                                                _ptr(hist, ctypes.c_uint64), ctypes.byref(bits)))
        return hist[:1 << bits.value].copy(), bits.value

    def shard_class_b(self, lo: int, hi: int, k: int, hist: np.ndarray, canonical: bool = False):
        """Class-B k-mers starting in [lo, hi) (gk_shard_class_b): (non-homopolymer starts uint32[m],
        homopolymer runs uint32[r, 3] = (first start, count, letter)); their ownership bins are added
        to ``hist`` (uint64, gk_shard_histogram's bins) in place.  ACGT-only sba: two empty arrays."""
        full = np.zeros(4096, dtype=np.uint64)
        full[:len(hist)] = hist
        nr, nh = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.lib.gk_shard_class_b(self.ctx, lo, hi, k, SORT_CANONICAL if canonical else 0,
                                              _ptr(full, ctypes.c_uint64), ctypes.byref(nr), ctypes.byref(nh)))
        hist[:] = full[:len(hist)]
        rest = np.empty(nr.value, dtype=np.uint32)
        runs = np.empty((nh.value, 3), dtype=np.uint32)
        self._check(self.lib.gk_shard_class_b_copy(self.ctx, _ptr(rest, ctypes.c_uint32), nr.value,
                                                   _ptr(runs, ctypes.c_uint32), nh.value))
        return rest, runs

    def shard_sort_range_b(self, k: int, digit_lo: int, digit_hi: int, rest: np.ndarray, runs: np.ndarray,
                           canonical: bool = False) -> int:
        """shard_sort_range with the class-B k-mers of the whole sba given (every rank's
        shard_class_b lists concatenated in rank order) instead of scanned for."""
        rest = np.ascontiguousarray(rest, dtype=np.uint32)
        runs = np.ascontiguousarray(runs, dtype=np.uint32).reshape(-1, 3)
        n = ctypes.c_uint64(0)
        self._check(self.lib.gk_shard_sort_range_b(self.ctx, k, SORT_CANONICAL if canonical else 0, digit_lo,
                                                   digit_hi, _ptr(rest, ctypes.c_uint32), len(rest),
                                                   _ptr(runs, ctypes.c_uint32), len(runs), ctypes.byref(n)))
        self.n = n.value
        return n.value

    def shard_sort_range(self, k: int, digit_lo: int, digit_hi: int, canonical: bool = False) -> int:
        """Sort the k-mers of the whole sequence whose top digit is in [digit_lo, digit_hi); returns
        their number (the context then holds them as after sort(k))."""
        n = ctypes.c_uint64(0)
        self._check(self.lib.gk_shard_sort_range(self.ctx, k, SORT_CANONICAL if canonical else 0, digit_lo, digit_hi,
                                                 ctypes.byref(n)))
        self.n = n.value
        return n.value

    def unique_count_only(self) -> int:
        g = ctypes.c_uint64(0)
        self._check(self.lib.gk_unique_counts(self.ctx, ctypes.byref(g)))
        return g.value

    def device_views(self):
        s, k, n, w = _P(), _P(), ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self.lib.gk_device_views(self.ctx, ctypes.byref(s), ctypes.byref(k), ctypes.byref(n),
                                             ctypes.byref(w)))
        return s.value, k.value, n.value, w.value

    def device_unique(self):
        """(device group starts u32*, device counts u32*, n_unique) of the last unique_counts."""
        g, c, n = _P(), _P(), ctypes.c_uint64()
        self._check(self.lib.gk_device_unique(self.ctx, ctypes.byref(g), ctypes.byref(c), ctypes.byref(n)))
        return g.value, c.value, n.value

    def materialize_keys(self) -> int:
        """Make the sorted keys resident (re-encoded from the sorted starts if the sort left them
        stale); returns the key words per k-mer."""
        s, k, n, w = _P(), _P(), ctypes.c_uint64(), ctypes.c_uint32()
        self._check(self.lib.gk_device_views(self.ctx, ctypes.byref(s), ctypes.byref(k), ctypes.byref(n),
                                             ctypes.byref(w)))
        return w.value

    def device_starts(self):
        """(device pointer of the current start indices, n) -- no key materialisation."""
        s, n = _P(), ctypes.c_uint64()
        self._check(self.lib.gk_device_views(self.ctx, ctypes.byref(s), None, ctypes.byref(n), None))
        return s.value, n.value

    def stream_handle(self) -> int:
        s = _P()
        self._check(self.lib.gk_stream(self.ctx, ctypes.byref(s)))
        return s.value or 0

    def profile_enable(self, on: bool = True):
        self._check(self.lib.gk_profile_enable(self.ctx, int(on)))

    def profile_report(self) -> dict:
        import json

        buf = ctypes.create_string_buffer(1 << 16)
        self._check(self.lib.gk_profile_report(self.ctx, buf, len(buf)))
        return json.loads(buf.value.decode())
