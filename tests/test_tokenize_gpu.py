"""tokenize_corpus_device (csrc/tokenize.hip) against tokenize_corpus: doc_ptr, tokens and terms
are equal exactly, on the fixtures of tests/tokenize_reference.py, random documents over a mixed
1- to 4-byte alphabet, the edges of a tile, forced hash collisions, and end to end through
TfidfFeatures. There is no tolerance anywhere."""
import numpy as np
import pytest

import tokenize_reference as ref
from graphconvgeo_amd import tfidf

pytestmark = pytest.mark.gpu
TILE = tfidf.TOKENIZE_TILE_BYTES
PATTERNS = list(tfidf.DEVICE_PATTERNS)


def check(cuda, texts, pattern=tfidf.TOKEN_PATTERN, stop_words=ref.STOPS, lowercase=True,
          vocabulary=None, **kw):
    want = tfidf.tokenize_corpus(texts, pattern, stop_words, lowercase, vocabulary)
    got = tfidf.tokenize_corpus_device(texts, pattern, stop_words, lowercase, vocabulary,
                                       device=cuda, **kw)
    assert isinstance(got[0], np.ndarray) and got[0].dtype == np.int64
    assert got[1].device.type == "cuda" and got[1].dtype.is_floating_point is False
    assert str(got[1].dtype) == "torch.int32" and got[1].ndim == 1
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    assert got[2] == want[2]
    return want


@pytest.fixture(scope="module")
def random_docs():
    return ref.random_texts(4242, 300)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("lowercase", [True, False])
def test_fixtures(cuda, pattern, lowercase):
    before = tfidf.tokenize_corpus_device.fallbacks
    want = check(cuda, ref.FIXTURES, pattern, lowercase=lowercase)
    assert len(want[2]) > 20
    plain = [t for t in ref.FIXTURES if "\x00" not in t]  # the documents found by their separators
    check(cuda, plain, pattern, lowercase=lowercase)
    assert tfidf.tokenize_corpus_device.fallbacks == before


@pytest.mark.parametrize("pattern", PATTERNS)
def test_random_documents(cuda, random_docs, pattern):
    plain = [t.replace("\x00", " ") for t in random_docs]
    want = check(cuda, plain, pattern)
    assert want[1].size > 500
    check(cuda, random_docs, pattern)  # with NULs inside documents: per-document offsets


def test_no_documents_and_empty_documents(cuda):
    check(cuda, [])
    check(cuda, [""])
    check(cuda, ["", "", ""])
    check(cuda, ["", "a", "", " ", "#ab"])       # bytes but no token
    check(cuda, ["the", "and of", ""])           # every token a stop word
    check(cuda, ["", "ab", ""])


def test_stop_lists(cuda, random_docs):
    for texts in (ref.FIXTURES, random_docs):
        check(cuda, texts, stop_words=None)
        check(cuda, texts, stop_words=ref.NON_ASCII_STOPS)
        check(cuda, texts, stop_words=["ab", "日本", "aa", "éé"])
    check(cuda, ["The quick brown fox and the lazy dog"], stop_words="english")


def test_fixed_vocabulary(cuda, random_docs):
    for texts in (ref.FIXTURES, random_docs):
        terms = tfidf.tokenize_corpus(texts, stop_words=None)[2]
        vocab = {t: i for i, t in enumerate(sorted(terms)[::2])}   # half the terms unseen
        vocab["the"] = len(vocab)                                  # a stop word in the vocabulary
        vocab["never-there"] = len(vocab)
        want = check(cuda, texts, vocabulary=vocab)
        assert want[2] is None and (want[1] == -1).any() and (want[1] >= 0).any()
        check(cuda, texts, vocabulary=vocab, stop_words=None)
        check(cuda, texts, vocabulary={})


def test_bytes_documents(cuda):
    texts = [t.encode("utf-8") if i % 2 else t for i, t in enumerate(ref.FIXTURES)]
    check(cuda, texts)
    with pytest.raises(UnicodeDecodeError):
        tfidf.tokenize_corpus_device([b"\xff\xfe"], device=cuda)
    with pytest.raises(ValueError, match="document 1 "):
        tfidf.tokenize_corpus_device(["ab", "cd \ud800"], stop_words=None, device=cuda)


def test_nul_inside_a_document(cuda):
    check(cuda, ["ab\x00cd", "ef"], stop_words=None)
    check(cuda, ["\x00", "\x00\x00ab", "cd\x00"], stop_words=None)
    check(cuda, ["#\x00ab @\x00cd x\x00y"], stop_words=None)


class Corpus:
    """Documents joined by one separator byte each, with the byte position kept, so that a
    document can be padded with spaces until something lands where a tile ends."""

    def __init__(self):
        self.texts, self.at = [], 0     # self.at = the byte at which the next document starts

    def add(self, text):
        self.texts.append(text)
        self.at += len(text.encode("utf-8")) + 1

    def add_straddling(self, unit, offset, head="pad "):
        """A document in which `unit` begins `offset` bytes from the next tile boundary that
        leaves room for `head`, after spaces, and is followed by a word."""
        target = (self.at + len(head) + 8 + TILE - 1) // TILE * TILE + offset
        text = head + " " * (target - self.at - len(head)) + unit + " tail"
        assert self.at + len((head + " " * (target - self.at - len(head))).encode()) == target
        self.add(text)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_tile_boundary(cuda, pattern):
    units = ["\U0001d400\U0001d401\U0001d402",   # 4-byte letters
             "\U0001f600ab\U0001f600",           # 4-byte non-word characters around a token
             "xy",                               # a two-character token
             "x y",                              # and one-character words
             "#tagged", "@me", "a#bc", "##xy",   # '#'-prefixed runs
             "é日本語ß"]
    c = Corpus()
    for unit in units:
        for offset in range(-4 - len(unit.encode()), 5):
            c.add_straddling(unit, offset)
    # a document separator at every offset around a boundary, tokens on both sides of it
    for offset in range(-4, 5):
        c.add_straddling("cd", offset - 2, head="ab ")
        c.texts[-1] = c.texts[-1][:-len(" tail")]
        c.at -= len(" tail")
        assert (c.at - 1) % TILE == offset % TILE    # where this document's separator is
        c.add("ef #gh")
        c.add("\U0001d400" * (1 + offset % 3) + "ij")
    assert c.at // TILE > 100 and "\x00" not in "".join(c.texts)
    want = check(cuda, c.texts, pattern, stop_words=None, lowercase=False)
    assert want[1].size > len(c.texts)
    # the same with a NUL inside one document: the documents by their byte offsets
    check(cuda, c.texts + ["x\x00y"], pattern, stop_words=None, lowercase=False)
    # and in one corpus whose last tile ends at every residue of 16
    for tail in range(17):
        check(cuda, [" " * (TILE - 8) + "abcdefgh", "x" * tail], pattern, stop_words=None)


def test_a_token_longer_than_a_tile(cuda):
    long = "ab" * TILE + "é" * 7
    want = check(cuda, ["x " + long + " y", long, "#" + long, long + "z"], stop_words=None)
    assert want[2] == [long, long + "z"]


def test_forced_collisions_fall_back_exactly(cuda, random_docs):
    before = tfidf.tokenize_corpus_device.fallbacks
    check(cuda, random_docs, hash_bits=3)
    assert tfidf.tokenize_corpus_device.fallbacks == before + 1
    check(cuda, ["ab ab ab", "ab"], stop_words=None, hash_bits=1)   # one term: nothing collides
    assert tfidf.tokenize_corpus_device.fallbacks == before + 1
    check(cuda, ref.FIXTURES, hash_bits=3, vocabulary={"tag": 0, "x_1": 1})
    assert tfidf.tokenize_corpus_device.fallbacks == before + 2
    check(cuda, random_docs, hash_bits=40)                           # cut, but wide enough
    assert tfidf.tokenize_corpus_device.fallbacks == before + 2


def synthetic_corpus(seed, n_docs):
    rng = np.random.default_rng(seed)
    words = ["w%d" % i for i in range(150)] + ["é%d" % i for i in range(30)] + \
        ["日本%d" % i for i in range(20)] + ["the", "and", "of"] + ["#t%d" % i for i in range(10)]
    p = 1.0 / np.arange(1, len(words) + 1)
    return [" ".join(rng.choice(words, size=int(rng.integers(0, 30)), p=p / p.sum()))
            for _ in range(n_docs)]


def test_features_end_to_end(cuda):
    from graphconvgeo_amd.tfidf import TfidfFeatures

    train, dev = synthetic_corpus(1, 200), synthetic_corpus(2, 60) + ["unseen words only", ""]
    kw = dict(min_df=2, max_df=0.5, stop_words=["the", "and", "of"], device=cuda)

    def run(tokenizer):
        vec = TfidfFeatures(tokenizer=tokenizer, **kw)
        a, b = vec.fit_transform(train), vec.transform(dev)
        return vec, [x.cpu().numpy() for m in (a, b) for x in (m.indptr, m.indices, m.data)]

    host, want = run("host")
    for _ in range(2):  # the second run is bitwise the first: both equal the host's
        vec, got = run("device")
        assert vec.feature_names_ == host.feature_names_ and len(vec.feature_names_) > 100
        assert np.array_equal(vec.df_.cpu().numpy(), host.df_.cpu().numpy())
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g.view(np.int32), w.view(np.int32))


def test_dataloader_features_passes_the_tokenizer(cuda):
    import pandas as pd

    from graphconvgeo_amd.tfidf import dataloader_features

    frames = [pd.DataFrame({"text": synthetic_corpus(s, n)}) for s, n in ((3, 120), (4, 30), (5, 30))]
    kw = dict(min_df=2, max_df=0.5, stop_words=None, device=cuda)
    X, vec = dataloader_features(*frames, tokenizer="device", **kw)
    Y, ref_vec = dataloader_features(*frames, **kw)
    assert vec.tokenizer == "device" and ref_vec.tokenizer == "host"
    assert vec.feature_names_ == ref_vec.feature_names_
    for a, b in ((X.indptr, Y.indptr), (X.indices, Y.indices), (X.data, Y.data)):
        assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
