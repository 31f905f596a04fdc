"""The byte rule of gcg_mention_mark against the regex engine, and mention_incidences rebuilt on
that rule (tests/mention_parse_reference.py) against mention_incidences itself. No GPU."""
import numpy as np
import pytest

import mention_parse_reference as ref
from graphconvgeo_amd import mentions
from graphconvgeo_amd.mentions import MENTION_PATTERN, mention_incidences


@pytest.mark.parametrize("text", ref.FIXTURES)
def test_rule_on_fixtures(text):
    assert ref.rule_findall(text) == MENTION_PATTERN.findall(text)


def test_fixtures_cover_both_outcomes():
    found = {t: MENTION_PATTERN.findall(t) for t in ref.FIXTURES}
    assert found["@ab"] == ["ab"] and found["@a"] == [] and found["@a1"] == ["a1"]
    assert found["@1a"] == [] and found["@_a"] == [] and found["@a_"] == ["a_"]
    assert found["a@bc"] == found[".@bc"] == found["-@bc"] == found["_@bc"] == []
    assert found["#@bc"] == found["@@bc"] == found["é@bc"] == ["bc"] and found["\n@ab"] == ["ab"]
    assert found["@bc@de"] == ["bc"] and found["@bc @de"] == ["bc", "de"]
    assert found["hello @"] == found["hello @a"] == [] and found["hello @ab"] == ["ab"]


def test_lowering_first_would_change_the_matches():
    kelvin, dotted = "x" + ref.KELVIN + "@ab", "@a" + ref.DOTTED_I + "b"
    assert MENTION_PATTERN.findall(kelvin) == ["ab"] and MENTION_PATTERN.findall(kelvin.lower()) == []
    assert MENTION_PATTERN.findall(dotted) == [] and MENTION_PATTERN.findall(dotted.lower()) == ["ai"]
    assert ref.rule_findall(kelvin) == ["ab"] and ref.rule_findall(dotted) == []


def test_rule_on_random_strings():
    texts = ref.random_strings(2024, 20000, 24)
    n_found = 0
    for t in texts:
        want = MENTION_PATTERN.findall(t)
        assert ref.rule_findall(t) == want, repr(t)
        n_found += len(want)
    assert n_found > 300
    # joined by NUL the texts are found as on their own: the '^' case through the separator
    joined = "\x00".join(t.replace("\x00", " ") for t in texts)
    assert ref.rule_findall(joined) == [m for t in texts
                                        for m in MENTION_PATTERN.findall(t.replace("\x00", " "))]


def same(got, want):
    assert got[0] == want[0] and got[1] == want[1]
    assert got[2].dtype == want[2].dtype and np.array_equal(got[2], want[2])
    assert got[3].dtype == want[3].dtype and np.array_equal(got[3], want[3])


def test_rule_incidences_on_the_golden_tables():
    tables = ref.golden_tables()
    want = mention_incidences(*tables)
    assert want[1] > want[0] and want[2].size > 100
    same(ref.rule_incidences(*tables), want)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rule_incidences_on_random_tables(seed):
    tables = ref.random_tables(seed)
    want = mention_incidences(*tables)
    assert want[1] > want[0] and (want[2] < want[0]).any() and (want[2] == want[3]).any()
    same(ref.rule_incidences(*tables), want)
    tables = ref.alphabet_tables(seed)
    same(ref.rule_incidences(*tables), mention_incidences(*tables))
    for tables in ref.one_user_tables(ref.FIXTURES):
        same(ref.rule_incidences(*tables), mention_incidences(*tables))


def test_the_device_parser_refuses_a_cpu_device():
    tables = ref.golden_tables()
    with pytest.raises(ValueError, match="CUDA"):
        mentions.mention_incidences_device(*tables, device="cpu")
    with pytest.raises(ValueError, match="parser"):
        mentions.mention_graph_operator(*tables, device="cpu", parser="gpu")
    with pytest.raises(ValueError, match="CUDA"):
        mentions.mention_graph_operator(*tables, device="cpu", parser="device")
    assert mentions.PARSERS == ("host", "device")


def test_the_new_entries_validate_before_any_launch(native_lib):
    import ctypes as C

    lib = native_lib
    nb = C.c_size_t()
    t16, f16, b8, w8 = (C.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000))
    assert lib.gcg_mention_mark_workspace_bytes(-1, C.byref(nb)) == 1
    assert lib.gcg_mention_mark_workspace_bytes(16, None) == 1
    assert "gcg_mention_mark_workspace_bytes" in lib.gcg_last_error().decode()
    mark = lib.gcg_mention_mark
    assert mark(-1, t16, f16, b8, b8, w8, 1 << 20, None) == 1                     # n_bytes
    assert mark(64, None, f16, b8, b8, w8, 1 << 20, None) == 1                    # no text
    assert mark(64, t16, f16, b8, b8, None, 0, None) == 1                         # no workspace
    assert mark(64, C.c_void_p(0x10004), f16, b8, b8, w8, 1 << 20, None) == 2     # text not 16-B
    assert "gcg_mention_mark" in lib.gcg_last_error().decode()
    terms = lib.gcg_tokenize_terms_folded
    args = (t16, f16, b8, 4, 2, None)
    out = (b8, b8, b8, b8, b8, w8, 1 << 20, None)
    assert terms(64, *args, 65, 1, *out) == 1                                     # hash_bits
    assert terms(6, *args, 64, 1, *out) == 1                                      # 4 names in 6 bytes
    assert terms(64, t16, C.c_void_p(0x20008), b8, 4, 2, None, 64, 1, *out) == 2  # flags not 16-B
    assert "gcg_tokenize_terms_folded" in lib.gcg_last_error().decode()
