"""A byte-level restatement of the run rule that csrc/tokenize.hip implements, and the fixtures
both its CPU check and the GPU tests use.

`findall` on (?u)\\b\\w\\w+\\b and (?u)(?<![#@])\\b\\w\\w+\\b is: a token is a maximal run of word
characters of at least two code points; with the lookbehind the run is dropped whole when the
code point before it is '#' or '@' (no later position inside a run is a \\b). Nothing here uses
`re` on the text: the word class comes in as the bitmap and the text as UTF-8 bytes."""
import numpy as np

STOPS = frozenset({"the", "and", "of", "to", "in", "is", "it"})
NON_ASCII_STOPS = frozenset({"stra\u00dfe", "\u03b1\u03c2", "\u65e5\u672c\u8a9e", "the"})

FIXTURES = [
    "#tag @user a#bc ##xy x_1 and #x @y_ z#@qq",
    "e\u0301 cafe\u0301 ne\u0301e",                          # a combining mark splits the run
    "\u0130stanbul \u0130\u0130 I\u0307",                   # \u0130 lowers to two code points
    "SS \u00df stra\u00dfe STRASSE",
    "\u0661\u0662\u0663 x\u00b2 \u00b2\u00b2 \u00bd\u00bd a\u0663",  # Arabic-Indic digits, superscript two
    "\u65e5\u672c\u8a9e \u3068 \u6f22\u5b57\u304b\u306a mixed\u6f22",  # CJK
    "\U0001d400\U0001d401 x\U0001d4d0 \U0001d7ce\U0001d7cf",  # 4-byte mathematical letters and digits
    "ab\U0001f600cd \U0001f600\U0001f600 a\U0001f600b",   # an emoji between letters
    "ab\u200dcd zw\u200d \u200d\u200d",                     # zero-width joiner
    "co\u00adop \u00ad\u00ad soft\u00ad",                   # soft hyphen
    "a b c I x",                                            # one-character words only
    "start of the document and its end",                    # a token at the start and at the end
    "",                                                     # an empty document
    "the and of to in is it",                               # only stop words
    "nul\x00inside #a\x00b \x00\x00 @\x00cd",             # NUL inside a document
    "\u0391\u03a3 \u03a3\u0391 \u0391\u03a3",               # final sigma in the middle and at the end
    "#",
    "@\u00e9\u00e9",
    "trailing \u0391\u03a3",                                # \u0391\u03a3 at a document's end
    "\u03a3",                                               # next document starts with a sigma
    "__ _ _a 9_ 0",
]


def word_at(table, cp):
    return bool((int(table[cp >> 5]) >> (cp & 31)) & 1) if cp < 0x110000 else False


def decode(buf, i):
    """(code point, byte length) of the character whose lead byte is buf[i]."""
    b0 = buf[i]
    if b0 < 0x80:
        return b0, 1
    if b0 < 0xE0:
        return ((b0 & 0x1F) << 6) | (buf[i + 1] & 0x3F), 2
    if b0 < 0xF0:
        return ((b0 & 0x0F) << 12) | ((buf[i + 1] & 0x3F) << 6) | (buf[i + 2] & 0x3F), 3
    return ((b0 & 7) << 18) | ((buf[i + 1] & 0x3F) << 12) | ((buf[i + 2] & 0x3F) << 6) | \
        (buf[i + 3] & 0x3F), 4


def token_spans(buf, doc_off, table, lookbehind):
    """[[(start byte, stop byte)] per document]: document d is buf[doc_off[d]:doc_off[d + 1] - 1]
    (one separator byte follows each document but the last, whose doc_off is len(buf) + 1)."""
    out = []
    for d in range(len(doc_off) - 1):
        i, end = int(doc_off[d]), int(doc_off[d + 1]) - 1
        spans, prev, run_start, run_chars, run_ok = [], None, -1, 0, False
        while i <= end:
            cp, n = decode(buf, i) if i < end else (None, 1)
            if cp is not None and word_at(table, cp):
                if run_start < 0:
                    run_start, run_chars = i, 0
                    run_ok = not (lookbehind and prev in (0x23, 0x40))
                run_chars += 1
            elif run_start >= 0:
                if run_chars >= 2 and run_ok:
                    spans.append((run_start, i))
                run_start = -1
            prev = cp
            i += n
        out.append(spans)
    return out


def corpus_bytes(texts, lowercase=True):
    """(buf, doc_off) with every document lowered on its own, joined by one NUL each."""
    parts = [(t.lower() if lowercase else t).encode("utf-8") for t in texts]
    doc_off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) + 1 for p in parts], out=doc_off[1:])
    return b"\x00".join(parts), doc_off


def tokenize(texts, table, lookbehind, stops=frozenset(), lowercase=True, vocabulary=None):
    """(doc_ptr, tokens, terms) under tokenize_corpus's contract, from the run rule."""
    buf, doc_off = corpus_bytes(texts, lowercase)
    fixed = vocabulary is not None
    ids = vocabulary if fixed else {}
    doc_ptr, tokens = np.zeros(len(texts) + 1, np.int64), []
    for d, spans in enumerate(token_spans(buf, doc_off, table, lookbehind)):
        for s, e in spans:
            w = buf[s:e].decode("utf-8")
            if w in stops:
                continue
            tokens.append(ids.get(w, -1) if fixed else ids.setdefault(w, len(ids)))
        doc_ptr[d + 1] = len(tokens)
    return doc_ptr, np.asarray(tokens, np.int32), None if fixed else list(ids)


ALPHABET = list("abAB zZ09_#@ .,-'\x00") + [
    "\u00e9", "\u00df", "\u0130", "\u03a3", "\u03c3", "\u0391", "\u0301", "\u00ad", "\u00b2",  # 2-byte
    "\u0661", "\u0e01", "\u200d", "\u65e5", "\u672c", "\u3001", "\u20ac",                      # 2- and 3-byte
    "\U0001d400", "\U0001d7ce", "\U0001f600", "\U00020000",                                    # 4-byte
]


def random_texts(seed, count, max_len=40):
    rng = np.random.default_rng(seed)
    return ["".join(rng.choice(ALPHABET, size=int(rng.integers(0, max_len + 1))))
            for _ in range(count)]
