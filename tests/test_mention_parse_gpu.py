"""mention_incidences_device (gcg_mention_mark, gcg_tokenize_terms_folded, the remap and the key
sort of gcg_tfidf_count) against mention_incidences: n_users, n_nodes, a and b are equal exactly,
on the fixtures of tests/mention_parse_reference.py, random tables, the edges of a tile and of
the corpus, forced hash collisions, and through the projection to the golden H. There is no
tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

import mention_parse_reference as ref
from graphconvgeo_amd import mentions, tfidf
from graphconvgeo_amd.mentions import mention_incidences, mention_incidences_device

pytestmark = pytest.mark.gpu
TILE = tfidf.TOKENIZE_TILE_BYTES
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def decoded(tables):
    """The tables with `bytes` texts decoded: what the host parser reads."""
    return [ref.frame(df.index, [t.decode("utf-8") if isinstance(t, bytes) else t
                                 for t in df["text"].tolist()]) for df in tables]


def check(cuda, tables, **kw):
    want = mention_incidences(*decoded(tables))
    got = mention_incidences_device(*tables, device=cuda, **kw)
    assert got[0] == want[0] and got[1] == want[1]
    for g, w in zip(got[2:], want[2:]):
        assert g.device.type == "cuda" and g.dtype == torch.int32 and g.ndim == 1
        assert g.is_contiguous() and np.array_equal(g.cpu().numpy(), w)
    return want


def train_only(users, texts):
    return ref.frame(users, texts), ref.frame([], []), ref.frame([], [])


def names(count):
    return ["usr%04d" % i for i in range(count)]


@pytest.fixture(scope="module")
def golden():
    return ref.golden_tables(), dict(np.load(os.path.join(GOLD, "mention_graph.npz")))


def test_fixtures_as_one_user_tables(cuda):
    before = mention_incidences_device.fallbacks
    found = 0
    for tables in ref.one_user_tables(ref.FIXTURES):
        found += check(cuda, tables)[2].size
    assert found == sum(len(mentions.MENTION_PATTERN.findall(t)) for t in ref.FIXTURES) > 8
    # and as the users of one table, mentioning each other
    users = ["ab", "bc", "de"] + names(len(ref.FIXTURES) - 3)
    check(cuda, ref.split3(users, ref.FIXTURES, (7, 15)))
    assert mention_incidences_device.fallbacks == before


def test_golden_tables(cuda, golden):
    want = check(cuda, golden[0])
    assert want[0] == int(golden[1]["n"]) and want[1] > want[0]


@pytest.mark.parametrize("seed", [1, 2])
def test_random_tables(cuda, seed):
    want = check(cuda, ref.random_tables(seed))
    assert want[1] > want[0] and (want[2] < want[0]).any()
    want = check(cuda, ref.alphabet_tables(seed))          # 300 users over the alphabet
    assert want[0] == 300 and want[2].size > 0


def test_names_hit_through_case_folding(cuda):
    users = ["usra00", "usrb01", "usrc02"]
    want = check(cuda, train_only(users, ["@USRB01 @UsrC02", "@USRA00 x", "@usra00 @USRA00 @Usra00"]))
    assert want[1] == want[0] and want[2].tolist() == [1, 2, 0, 0] and want[3].tolist() == [0, 0, 1, 2]


def test_one_id_for_both_spellings_of_an_external_name(cuda):
    users = names(4)
    texts = ["@Second @FIRST_ext", "@first_EXT @usr0003", "@first_ext @SECOND @third", "@THIRD @second"]
    want = check(cuda, ref.split3(users, texts, (2, 3)))
    # numbered where the first spelling appears: second = 4, first_ext = 5, third = 6
    assert want[1] == 7 and want[2].tolist() == [4, 5, 3, 5, 4, 5, 6, 4, 6]


def test_nul_inside_a_text(cuda):
    users = names(4)
    check(cuda, train_only(users, ["@ab\x00@cd", "x\x00@ab", "@a\x00b @usr0000", "\x00"]))
    check(cuda, ref.split3(users, ["\x00@ab", "-\x00@cd", "@ab\x00", "@cd"], (1, 2)))
    for tables in ref.one_user_tables(ref.random_strings(5, 40, 30)):   # NUL is in the alphabet
        check(cuda, tables)


def test_empty_texts_no_users_and_no_mentions(cuda):
    empty = ref.frame([], [])
    got = mention_incidences_device(empty, empty, empty, device=cuda)
    assert got[:2] == (0, 0) and got[2].numel() == got[3].numel() == 0
    check(cuda, (empty, empty, empty))
    check(cuda, train_only(["solo"], [""]))
    check(cuda, train_only(names(3), ["", "", ""]))
    check(cuda, ref.split3(names(4), ["", "no mention @ all", "a@bc .@de", "@1x"], (1, 3)))
    check(cuda, ref.split3(names(4), ["", "@usr0003", "", ""], (1, 3)))
    with pytest.raises(ValueError, match="duplicate target node"):
        mention_incidences_device(*ref.split3(["a", "b", "a"], ["", "", ""], (1, 2)), device=cuda)


def test_bytes_texts(cuda):
    users = names(len(ref.FIXTURES))
    texts = [t.encode("utf-8") if i % 2 else t for i, t in enumerate(ref.FIXTURES)]
    check(cuda, ref.split3(users, texts, (5, 9)))
    before = mention_incidences_device.fallbacks
    check(cuda, ref.split3(users, texts, (5, 9)), hash_bits=1)          # through the fallback too
    assert mention_incidences_device.fallbacks == before + 1


class Corpus:
    """Users whose texts are joined by one separator byte each, with the byte position kept, so
    that a text can be padded with spaces until something lands where a tile ends."""

    def __init__(self):
        self.texts, self.at = [], 0     # self.at = the byte at which the next text starts

    def add(self, text):
        self.texts.append(text)
        self.at += len(text.encode("utf-8")) + 1

    def add_at(self, unit, offset, tail=" tail"):
        """A text in which `unit` begins `offset` bytes from the next tile boundary with room
        before it, after spaces."""
        target = (self.at + 16 + TILE - 1) // TILE * TILE + offset
        self.add(" " * (target - self.at) + unit + tail)

    def tables(self):
        return train_only(names(len(self.texts)), self.texts)


def test_tile_boundary(cuda):
    c = Corpus()
    # '@' at every offset from -3 to +3 of a boundary, so that the byte before it and the two
    # after it fall on either side: before it a byte of P, of neither class, or the two bytes of
    # a code point; after it names, and what is no name
    for before in (" ", ".", "_", "a", "é", "#"):
        for after in ("ab", "Ab9", "a", "a ", "1a", "a-b", "a_", "_a", "éb"):
            for offset in range(-3, 4):
                c.add_at(before + "@" + after, offset - len(before.encode("utf-8")))
    # a text that begins with the '@' there (the '^' case through the separator), after a text
    # that ends in a byte of P
    for offset in range(-3, 4):
        c.add_at("x.", offset - 3, tail="")
        assert (c.at - TILE) % TILE == offset % TILE
        c.add("@ab and @usr0001")
    # names that cross the boundary at each of their bytes
    for offset in range(-9, 1):
        c.add_at("@Crossing", offset)
    assert c.at // TILE > 350
    want = check(cuda, c.tables())
    assert want[2].size > 80 and want[1] > want[0]


def test_a_name_longer_than_a_tile(cuda):
    long = "aB" * TILE
    want = check(cuda, train_only(names(4), ["x @" + long + " y", "@" + long.lower(), "-@" + long,
                                             "@" + long.upper() + "z @" + long.swapcase()]))
    assert want[1] == want[0] + 2 and want[2].tolist() == [4, 4, 4, 5]


def test_corpus_ending_at_every_residue_of_16(cuda):
    for tail in range(16):
        for end, found in (("@", 0), ("@a", 0), ("@ab", 1)):
            text = " " * (TILE - 8 + tail) + end
            texts = ["@usr0001", text[len("@usr0001") + 1:]]      # the corpus is len(text) bytes
            want = check(cuda, train_only(names(2), texts))
            assert want[2].size == 1 + found


def test_text_boundary_directly_before_a_mention(cuda):
    for last in ("a", "9", "_", ".", "-"):
        want = check(cuda, ref.split3(names(3), ["x" + last, "@ab", "@ab" + last], (1, 2)))
        assert want[2].size == 2
        assert mentions.MENTION_PATTERN.findall("x" + last + "@ab") == []


def test_forced_collisions_fall_back_exactly(cuda):
    tables = ref.random_tables(7)
    before = mention_incidences_device.fallbacks
    check(cuda, tables, hash_bits=3)
    assert mention_incidences_device.fallbacks == before + 1
    check(cuda, train_only(names(2), ["@ab @AB @Ab", "@aB"]), hash_bits=1)   # one name: no collision
    assert mention_incidences_device.fallbacks == before + 1
    # names equal but for case are one term; names that differ after folding collide
    check(cuda, train_only(names(2), ["@ab @AB", "@ac @ad"]), hash_bits=1)   # three names, two hashes
    assert mention_incidences_device.fallbacks == before + 2
    check(cuda, tables, hash_bits=40)
    assert mention_incidences_device.fallbacks == before + 2


def test_two_calls_give_identical_tensors(cuda):
    tables = ref.random_tables(11, 200)
    first = mention_incidences_device(*tables, device=cuda)
    timings = {}
    second = mention_incidences_device(*tables, device=cuda, timings=timings)
    assert first[:2] == second[:2]
    assert torch.equal(first[2], second[2]) and torch.equal(first[3], second[3])
    assert set(timings) == {"prep_s", "upload_s", "kernels_s", "terms_s"}


def test_projection_takes_the_device_tensors(cuda, golden):
    tables, gold = golden
    n_users, n_nodes, a, b = mention_incidences_device(*tables, device=cuda)
    u, v = mentions.project_mentions(n_users, n_nodes, a, b, 10, cuda)
    got = np.stack([u.cpu().numpy(), v.cpu().numpy()], axis=1)
    assert np.array_equal(got, gold["edges"])


def test_operator_with_the_device_parser_is_the_golden_H(cuda, golden):
    tables, gold = golden
    H = mentions.mention_graph_operator(*tables, celebrity_threshold=10, device=cuda, parser="device")
    host = mentions.mention_graph_operator(*tables, celebrity_threshold=10, device=cuda, parser="host")
    for got, want, other in ((H.indptr, gold["H_indptr"], host.indptr),
                             (H.indices, gold["H_indices"], host.indices),
                             (H.data, gold["H32_data"], host.data)):
        g = got.cpu().numpy()
        assert g.dtype == want.dtype and np.array_equal(g.view(np.int32), want.view(np.int32))
        assert np.array_equal(g.view(np.int32), other.cpu().numpy().view(np.int32))


def test_the_tokeniser_still_equals_the_host(cuda):
    import tokenize_reference as tok

    texts = tok.random_texts(4242, 300)
    for pattern in tfidf.DEVICE_PATTERNS:
        want = tfidf.tokenize_corpus(texts, pattern, tok.STOPS)
        got = tfidf.tokenize_corpus_device(texts, pattern, tok.STOPS, device=cuda)
        assert np.array_equal(got[0], want[0]) and got[2] == want[2]
        assert np.array_equal(got[1].cpu().numpy(), want[1])
