"""`map` with the trim in front (map_reads(trim=...), dph_map_run_trim) without a GPU: the arguments that are refused before any device
call, the host expectation the GPU test holds the reverse strands to - checked here against the packer on ASCII reverse complements -
and the whole-run test's inputs, which must be such that a run that skipped the trim cannot pass.  Integers and text: equal means equal."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import trim_cases as TC
from tests import trim_mid_model as MM
from tests import trim_model as M
from tests.test_overlap_trim_cpu import GEN, generate, reads_of, written

# the map flags of the GPU test (tests/test_map_trim_gpu.py); everything else is the command's default
MAP = dict(k=11)
MIN_LENGTH = 500
# source reads of the kernel test: 64 bases = 16 packed bytes, the boundary every read starts on; the last one spans many workgroups
SRC_LENS = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000, 70_001]
ALPHABET = b"ACGTACGTACGTacgtNnUuRY"  # (the mixed alphabet of test_overlap_trim_gpu._sources)


def pack(seq):
    """dph_pack_bases of a host slice: ceil(n / 4) bytes, first base in a byte's top bits, the last byte's unused bits zero"""
    from downpore_amd.overlap import load_host
    H = load_host()
    H.dph_pack_bases.restype = None
    H.dph_pack_bases.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int]
    out = np.zeros((len(seq) + 3) // 4, dtype=np.uint8)
    if len(seq):
        H.dph_pack_bases(bytes(seq), len(seq), out.ctypes.data, 0)
    return out


def codes_of(packed, n):
    """the n 2-bit codes of a packed read"""
    p = np.asarray(packed, dtype=np.uint8)
    return np.stack([(p >> 6) & 3, (p >> 4) & 3, (p >> 2) & 3, p & 3], axis=1).reshape(-1)[:n]


def pack_codes(codes):
    c = np.zeros((len(codes) + 3) // 4 * 4, dtype=np.uint8)
    c[:len(codes)] = codes
    c = c.reshape(-1, 4)
    return ((c[:, 0] << 6) | (c[:, 1] << 4) | (c[:, 2] << 2) | c[:, 3]).astype(np.uint8)


def reverse_strand(packed, n):
    """the reverse complement of a packed read of n bases, computed from its codes: reversed, 3 - code, repacked"""
    return pack_codes((3 - codes_of(packed, n)[::-1]).astype(np.uint8))


def sources(alphabet=ALPHABET, seed=91):
    rng = np.random.default_rng(seed)
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return [a[rng.integers(0, len(a), n)].tobytes() for n in SRC_LENS]


def reference():
    """the genome the generated reads were drawn from, as the reference read set of both the oracle and the product"""
    return np.frombuffer(O.gen_genome(GEN["seed"], GEN["genome"]), dtype=np.uint8), np.array([0, GEN["genome"]], dtype=np.int64)


# ---- refused before any library call / any device call ---------------------------------------------------------------------------
def test_map_reads_names_what_a_trim_dict_lacks_or_does_not_know():
    from downpore_amd.hip import DpError
    from downpore_amd.mapping import map_reads
    ads = object()  # (never touched: the dict is checked before anything is loaded)
    with pytest.raises(DpError, match="'front'"):
        map_reads(None, None, trim=dict(back=ads))
    with pytest.raises(DpError, match="'back'"):
        map_reads(None, None, trim=dict(front=ads, k=6))
    with pytest.raises(DpError, match="'front' and 'back'"):
        map_reads(None, None, trim=dict(k=6))
    with pytest.raises(DpError, match="unknown trim key 'midle'"):
        map_reads(None, None, trim=dict(front=ads, back=ads, midle=True))
    with pytest.raises(DpError, match="dict"):
        map_reads(None, None, trim=True)


def test_dph_map_run_trim_refuses_bad_arguments_with_a_text():
    from downpore_amd.overlap import Reads, load_host
    H = load_host()
    vp = C.c_void_p
    H.dph_map_run_trim.restype = vp
    H.dph_map_run_trim.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(vp)]
    H.dph_last_error.restype = C.c_char_p
    H.dph_last_error.argtypes = [vp]
    g, off = reference()
    ref = Reads(g[:5000], np.array([0, 5000], dtype=np.int64), min_len=0, himem=False)
    raw = Reads(g[:5000], np.array([0, 2000, 5000], dtype=np.int64), min_len=50, himem=False)
    front, back = reads_of(TC.FRONT, 0), reads_of(TC.BACK, 0)
    tp = np.array([6, 10000, 90, 5, 1, 0, 1, 1, 1, 5000, 85, 100, 0, 300_000_000], dtype=np.int64)
    mp = np.array([1, 11, 1000, 500, 10000, 40, 0, 0], dtype=np.int64)

    def run(handles=(ref.h, raw.h, front.h, back.h), trim=tp.ctypes.data, n_trim=14, params=mp.ctypes.data, n_params=8, out=True):
        th = vp(0x1234)
        h = H.dph_map_run_trim(*handles, trim, n_trim, params, n_params, 0, C.byref(th) if out else None)
        assert not h and (not out or not th.value)  # NULL, and no trim handle either
        return H.dph_last_error(None).decode()

    for i in range(4):
        hs = [ref.h, raw.h, front.h, back.h]
        hs[i] = None
        assert run(handles=hs).startswith("dph_map_run_trim: bad arguments")
    assert run(trim=None).startswith("dph_map_run_trim: bad arguments")
    assert run(out=False).startswith("dph_map_run_trim: bad arguments")
    for n in (0, 7, 9, 13, 15):
        assert "8 trim parameters, or 14" in run(n_trim=n)
    assert run(params=None).startswith("dph_map_run_trim: bad arguments")
    for n in (0, 5, 9):
        assert "6, 7 or 8 parameters" in run(n_params=n)
    mp[6] = 3
    assert "index layout 3" in run()
    mp[6], mp[7] = 0, 2
    assert "all sequences 2" in run()


# ---- the GPU test's expectation for a reverse strand -------------------------------------------------------------------------------
def _revcomp(seq):
    return bytes(seq).translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def test_the_reverse_strand_from_codes_is_the_packer_on_the_ascii_reverse_complement():
    for s in sources(alphabet=b"ACGT", seed=5):
        n = len(s)
        p = pack(s)
        assert np.array_equal(pack_codes(codes_of(p, n)), p)  # unpack / repack is the identity
        got = reverse_strand(p, n)
        assert np.array_equal(got, pack(_revcomp(s))), n
        if n % 4:
            assert got[-1] & ((1 << (2 * (4 - n % 4))) - 1) == 0  # unused bits zero
        assert np.array_equal(reverse_strand(got, n), p)
    # slices at every alignment, as the kernel test cuts them
    s = sources(alphabet=b"ACGT", seed=6)[10]
    for start in range(16):
        for ln in (1, 15, 16, 17, 63, 64, 65, len(s) - start):
            cut = s[start:start + ln]
            assert np.array_equal(reverse_strand(pack(cut), ln), pack(_revcomp(cut))), (start, ln)


# ---- the whole-run test's inputs -------------------------------------------------------------------------------------------------
def test_the_whole_run_inputs_are_not_vacuous(tmp_path):
    """Measured with the models and the oracle: the middle-stage model's output keeps 293 reads and maps to 294 PAF lines with
    _(left) and _(right) halves among them, the edge model's keeps 299 and maps to 299 lines, the untrimmed file maps to 299 lines
    that differ from both."""
    names, seqs, quals, kinds = generate(fastq=False, **GEN)
    path = str(tmp_path / "reads.fasta")
    TC.write_fasta(path, names, seqs, quals)
    g, off = reference()
    ref = O.ReadSet(g, off, min_len=0, himem=False)
    pafs = {}
    for tag, m in (("middle", MM.run(path, k=6)), ("edges", M.run(path, k=6))):
        trimmed = O.ReadSet(fasta=written(tmp_path, m, False, tag), min_len=MIN_LENGTH, himem=False)
        pafs[tag], _ = O.map_run(ref, trimmed, min_length=MIN_LENGTH, **MAP)
        print(tag, "reads kept", len(trimmed), "PAF lines", pafs[tag].count("\n"))
        assert 100 < len(trimmed) <= len(names) + 20
        assert pafs[tag].count("\n") > 100
    pafs["raw"], _ = O.map_run(ref, O.ReadSet(fasta=path, min_len=MIN_LENGTH, himem=False), min_length=MIN_LENGTH, **MAP)
    print("raw PAF lines", pafs["raw"].count("\n"))
    assert pafs["raw"].count("\n") > 100
    assert "_(left)" in pafs["middle"] and "_(right)" in pafs["middle"]
    assert "_(left)" not in pafs["edges"] and "_(right)" not in pafs["edges"]
    assert pafs["raw"] != pafs["middle"] and pafs["raw"] != pafs["edges"] and pafs["middle"] != pafs["edges"]
