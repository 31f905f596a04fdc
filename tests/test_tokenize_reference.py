"""The host side of the device tokeniser, without a GPU: the word-class bitmap against `re`, the
run rule (tests/tokenize_reference.py, what csrc/tokenize.hip implements) against
tokenize_corpus, the corpus buffer, and the argument checks."""
import re

import numpy as np
import pytest

import tokenize_reference as ref
from graphconvgeo_amd import tfidf

PATTERNS = [(tfidf.TOKEN_PATTERN, 1), (tfidf.SKLEARN_TOKEN_PATTERN, 0)]


def same(a, b):
    assert np.array_equal(a[0], b[0]) and a[0].dtype == b[0].dtype == np.int64
    assert np.array_equal(a[1], b[1]) and a[1].dtype == b[1].dtype == np.int32
    assert a[2] == b[2]


def test_word_char_table_is_the_regex_engines_word_class():
    table = tfidf.word_char_table()
    assert table.dtype == np.uint32 and table.shape == (0x110000 // 32,)
    assert tfidf.word_char_table() is table
    bits = np.unpackbits(table.view(np.uint8), bitorder="little")
    word = re.compile(r"(?u)\w")
    want = np.fromiter((word.fullmatch(chr(cp)) is not None for cp in range(0x110000)), bool,
                       0x110000)
    assert np.array_equal(bits.astype(bool), want)
    assert int(bits.sum()) > 100_000 and not bits[0] and bits[ord("_")] and not bits[ord("#")]


def test_supported_patterns_and_tile():
    assert tfidf.DEVICE_PATTERNS == {tfidf.TOKEN_PATTERN: 1, r"(?u)\b\w\w+\b": 0}
    assert tfidf.TOKENIZE_TILE_BYTES == 4096


@pytest.mark.parametrize("pattern,lookbehind", PATTERNS)
@pytest.mark.parametrize("lowercase", [True, False])
def test_run_rule_equals_findall_on_the_fixtures(pattern, lookbehind, lowercase):
    table = tfidf.word_char_table()
    for stops in (frozenset(), ref.STOPS, ref.NON_ASCII_STOPS):
        want = tfidf.tokenize_corpus(ref.FIXTURES, pattern, stops, lowercase)
        same(ref.tokenize(ref.FIXTURES, table, lookbehind, stops, lowercase), want)
        vocab = {t: i for i, t in enumerate(sorted(want[2])[::2])}
        same(ref.tokenize(ref.FIXTURES, table, lookbehind, stops, lowercase, vocab),
             tfidf.tokenize_corpus(ref.FIXTURES, pattern, stops, lowercase, vocab))


@pytest.mark.parametrize("pattern,lookbehind", PATTERNS)
@pytest.mark.parametrize("lowercase", [True, False])
def test_run_rule_equals_findall_on_random_strings(pattern, lookbehind, lowercase):
    table = tfidf.word_char_table()
    texts = ref.random_texts(20260 + lookbehind, 3000)
    assert {len(c.encode()) for t in texts for c in t} == {1, 2, 3, 4}
    same(ref.tokenize(texts, table, lookbehind, ref.STOPS, lowercase),
         tfidf.tokenize_corpus(texts, pattern, ref.STOPS, lowercase))


def test_corpus_buffer_lowers_each_document_as_on_its_own():
    plain = [t for t in ref.FIXTURES + ref.random_texts(5, 500) if "\x00" not in t]
    buf, doc_off = tfidf._corpus_bytes(plain, True)
    assert doc_off is None and buf == ref.corpus_bytes(plain, True)[0]
    assert "ας".encode() + b"\x00" in buf  # the final sigma before a separator
    buf, doc_off = tfidf._corpus_bytes(ref.FIXTURES, True)  # one document holds NULs
    want_buf, want_off = ref.corpus_bytes(ref.FIXTURES, True)
    assert buf == want_buf and np.array_equal(doc_off, want_off)
    buf, doc_off = tfidf._corpus_bytes([b"caf\xc3\xa9 AB", "x"], False)
    assert buf == "café AB\x00x".encode() and doc_off is None


def test_unsupported_pattern_names_the_host_tokeniser():
    for pattern in (r"\w+", r"(?u)\b\w+\b", r"(?u)(?<![#@])\b\w\w+\b "):
        with pytest.raises(ValueError, match="tokenize_corpus"):
            tfidf.tokenize_corpus_device(["ab cd"], token_pattern=pattern, stop_words=None)
        with pytest.raises(ValueError, match="tokenize_corpus"):
            tfidf.TfidfFeatures(token_pattern=pattern, tokenizer="device")
    tfidf.TfidfFeatures(token_pattern=r"\w+")  # the host tokeniser takes any pattern


def test_tokenizer_argument():
    assert tfidf.TfidfFeatures().tokenizer == "host"
    assert tfidf.TfidfFeatures(tokenizer="device").tokenizer == "device"
    for bad in ("gpu", "cuda", None, ""):
        with pytest.raises(ValueError, match="tokenizer"):
            tfidf.TfidfFeatures(tokenizer=bad)


def test_bad_documents_raise_before_the_device_is_touched():
    with pytest.raises(ValueError, match="document 1 "):
        tfidf._corpus_bytes(["fine", "lone \ud800 surrogate"], True)
    with pytest.raises(ValueError, match="document 1 "):
        tfidf._corpus_bytes(["nul \x00 here", "lone \udfff surrogate"], True)
    with pytest.raises(ValueError, match="document 2 is not a string"):
        tfidf._corpus_bytes(["a", b"b", 3], True)
    with pytest.raises(ValueError, match="device must be"):
        tfidf.tokenize_corpus_device(["ab"], stop_words=None, device="cpu")
    with pytest.raises(ValueError, match="hash_bits"):
        tfidf.tokenize_corpus_device(["ab"], stop_words=None, hash_bits=0)


def test_abi_argument_validation_without_gpu(native_lib):
    """The tokenising entries validate on the host before any launch."""
    import ctypes as C
    lib = native_lib
    nb = C.c_size_t()
    a16, b16, c16, d16 = (C.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000))
    assert lib.gcg_tokenize_tile_bytes() == tfidf.TOKENIZE_TILE_BYTES
    assert lib.gcg_tokenize_mark_workspace_bytes(-1, C.byref(nb)) == 1
    assert lib.gcg_tokenize_mark_workspace_bytes((1 << 33) + 1, C.byref(nb)) == 1
    assert lib.gcg_tokenize_mark(64, None, b16, 1, c16, d16, a16, a16, 1 << 20, None) == 1
    assert lib.gcg_tokenize_mark(64, C.c_void_p(0x10004), b16, 1, c16, d16, a16, a16, 1 << 20,
                                 None) == 2
    assert lib.gcg_tokenize_terms_workspace_bytes(10, 0, C.byref(nb)) == 1
    assert lib.gcg_tokenize_terms_workspace_bytes(10, 65, C.byref(nb)) == 1
    assert lib.gcg_tokenize_terms(64, a16, b16, c16, 40, 1, None, 64, d16, d16, d16, d16, d16, a16,
                                  1 << 20, None) == 1  # 40 tokens do not fit 64 bytes
    assert lib.gcg_tokenize_terms(64, a16, b16, c16, 4, 0, None, 64, d16, d16, d16, d16, d16, a16,
                                  1 << 20, None) == 1  # no document
    assert lib.gcg_tokenize_remap(4, a16, 5, b16, 1, c16, d16, d16, a16, 1 << 20, None) == 1
    assert "gcg_tokenize_remap" in lib.gcg_last_error().decode()
