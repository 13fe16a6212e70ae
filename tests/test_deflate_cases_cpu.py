"""The deflate cases themselves, without a GPU: the restatement of 'pgnn
deflate v1' (tests/_deflate_cases.py) writes streams zlib accepts, its
Adler-32 and its length bound hold, and every case reaches the branch it is
named for."""
import zlib

import numpy as np
import pytest

import _deflate_cases as DC

CASES = DC.cases()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def encoded():
    return {c.name: DC.reference(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_zlib_inflates_the_restatement(case, encoded):
    data, _ = encoded[case.name]
    s = DC.scanlines(case.image).tobytes()
    assert data[:2] == b"\x78\x01"
    assert zlib.decompress(data) == s
    assert int.from_bytes(data[-4:], "big") == zlib.adler32(s)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_reaches_its_branch(case, encoded):
    _, tokens = encoded[case.name]
    s = DC.scanlines(case.image)
    # the tokens tile every chunk
    for k, toks in enumerate(tokens):
        pos = k * case.chunk
        for t in toks:
            assert t.pos == pos and (t.dist == 0) == (t.length == 1)
            pos += t.length
        assert pos == min(len(s), (k + 1) * case.chunk)
    case.check(tokens, s, case.chunk, 1 + 3 * case.image.shape[1])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_length_is_within_the_capacity(case, encoded):
    data, _ = encoded[case.name]
    h, w = case.image.shape[:2]
    assert len(data) <= DC.capacity(h, w, case.chunk)


def test_noise_fills_its_slots():
    """All-9-bit literals: only the filter bytes' missing bit per row and the
    last chunk's unused stored block separate the stream from the bound."""
    case = {c.name: c for c in CASES}["noise_worst_case_slot"]
    data, _ = DC.deflate(case.image, case.chunk)
    h, w = case.image.shape[:2]
    slack = DC.capacity(h, w, case.chunk) - len(data)
    assert 0 <= slack <= 5 + (h + 7) // 8 + len(range(0, h * (3 * w + 1),
                                                      case.chunk))


def test_a_match_never_costs_more_than_its_literals():
    """The slot formula counts 9 bits per byte: the dearest match, length 3
    at a distance with 13 extra bits, is 7 + 5 + 13 bits."""
    for length in range(3, 259):
        k, _ = DC.length_code(length)
        bits = (7 if k < 23 else 8) + DC.LEN_EXTRA[k] + 5 + 13
        assert bits <= 9 * length


def test_adler_combine_is_adler32_of_the_concatenation():
    rng = np.random.RandomState(3)
    data = rng.randint(0, 256, 70000).astype(np.uint8).tobytes()
    data = data[:30000] + b"\xff" * 20000 + data[30000:]
    for cuts in ((1,), (256, 512), (32768, 65536), (5, 6, 89999),
                 tuple(range(4096, 90000, 4096))):
        pair, prev = (1, 0), 0
        for cut in cuts + (len(data),):
            part = data[prev:cut]
            pair = DC.adler_combine(pair, DC.adler_pair(part), len(part))
            prev = cut
        assert pair[1] << 16 | pair[0] == zlib.adler32(data)
    a, b = DC.adler_pair(data[:1000])
    assert b << 16 | a == zlib.adler32(data[:1000])
