"""CPU: the COCO run-length format.  The literal vectors of the contract (worked by hand from the rules: see each test), the naive
restatement in tests/_rle_reference.py against itself (round trips), and the host helpers of maskunet_amd.rle against it."""
import numpy as np
import pytest

from tests import _rle_reference as R

SIZES = [(1, 1), (1, 7), (7, 1), (5, 7), (16, 16)]


def _helpers():
    from maskunet_amd import rle
    return rle.rle_string_from_counts, rle.rle_counts_from_string


def _masks(H, W):
    rng = np.random.default_rng(100 * H + W)
    out = [np.zeros((H, W), bool), np.ones((H, W), bool)]
    for p in (0.1, 0.5, 0.9):
        out += [rng.random((H, W)) < p for _ in range(4)]
    return out


def test_literal_vectors():
    """3x3, centre pixel: column-major position 1 * 3 + 1 = 4 -> 4 zeros, 1 one, 4 zeros; each value is below 16, so one character
    48 + value each.  16 = 0b10000: c = 16, x = 0, bit 4 is set and x != -1 -> more, chr(48 + 48) = '`'; then c = 0, x = 0 -> '0'.
    -1: c = 31, x = -1, bit 4 set and x == -1 -> done, chr(48 + 31) = 'O'.  0: '0'.
    16384 = 16 << 10: two groups of zeros with more ('P' = 48 + 32), then 16 -> '`', then '0'.  65536 = 2 << 15: three 'P', then '2'."""
    m = np.zeros((3, 3), bool)
    m[1, 1] = True
    assert R.encode(m) == [4, 1, 4] and R.string([4, 1, 4]) == "414"
    assert R.string([16]) == "`0"
    assert R.string([5, 5, 5, 4]) == "555O"            # the fourth count is stored as 4 - 5 = -1
    assert R.string([5, 5, 5, 5]) == "5550"            # ... and as 5 - 5 = 0
    assert R.encode(np.zeros((128, 128), bool)) == [16384] and R.string([16384]) == "PP`0"
    assert R.encode(np.zeros((256, 256), bool)) == [65536] and R.string([65536]) == "PPP2"
    assert R.area([4, 1, 4]) == 1 and R.area([16384]) == 0 and R.area([0, 9]) == 9


def test_literal_vectors_through_the_host_helpers():
    to_s, to_c = _helpers()
    assert to_s([4, 1, 4]) == "414" and to_c("414") == [4, 1, 4]
    assert to_s([16]) == "`0" and to_s([5, 5, 5, 4]) == "555O" and to_s([5, 5, 5, 5]) == "5550"
    assert to_s([16384]) == "PP`0" and to_s([65536]) == "PPP2"
    assert to_c("PP`0") == [16384] and to_c("PPP2") == [65536] and to_c("555O") == [5, 5, 5, 4] and to_c(b"5550") == [5, 5, 5, 5]
    assert to_s([]) == "" and to_c("") == []


def test_walk_is_column_major():
    m = np.zeros((5, 7), bool)
    m[2, 0] = m[3, 0] = m[0, 1] = True                 # positions 2, 3 and 1 * 5 + 0 = 5
    assert R.encode(m) == [2, 2, 1, 1, 29]
    # transposed, [7,5]: the pixels are (y=0,x=2), (0,3), (1,0) -> positions 2 * 7 = 14, 3 * 7 = 21 and 1
    assert R.encode(m.T.copy()) == [1, 1, 12, 1, 6, 1, 13]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_trips(size):
    H, W = size
    to_s, to_c = _helpers()
    for m in _masks(H, W):
        c = R.encode(m)
        assert c == R.encode_fast(m)
        assert sum(c) == H * W and all(v > 0 for v in c[1:]) and c[0] >= 0
        assert R.area(c) == int(m.sum())
        s = R.string(c)
        assert R.parse(s) == c
        assert np.array_equal(R.decode(c, H, W), m)
        assert to_s(c) == s and to_c(s) == c
        assert all(48 <= ord(ch) < 112 for ch in s)


def test_strings_of_signed_values():
    """every count and every difference up to +-65536 takes at most 4 characters and survives the round trip"""
    to_s, to_c = _helpers()
    rng = np.random.default_rng(3)
    edge = [0, 1, 15, 16, 31, 32, 511, 512, 16383, 16384, 65535, 65536]
    for a in edge:
        for b in edge:
            c = [3, 7, a, 9, b]                        # b is stored as b - a: both signs, 0 and +-65536 included
            s = R.string(c)
            assert R.parse(s) == c and to_s(c) == s and to_c(s) == c
            assert len(s) <= 2 + 4 + 1 + 4
    for _ in range(200):
        c = rng.integers(0, 65537, size=int(rng.integers(1, 12))).tolist()
        s = R.string(c)
        assert len(s) <= 4 * len(c) and R.parse(s) == c and to_s(c) == s and to_c(s) == c


def test_decode_rejects_counts_that_do_not_cover_the_image():
    assert R.decode([4, 1, 4], 3, 3) is not None
    assert R.decode([4, 1, 3], 3, 3) is None and R.decode([4, 1, 5], 3, 3) is None and R.decode([], 3, 3) is None
    assert R.decode([10, -1, 0], 3, 3) is None          # sums to 9, but a count is negative
    off = np.array([[0, 3, 6, 9, 9]], np.int32)
    cnt = np.array([[4, 1, 4, 4, 1, 3, 10, -1, 0, 0, 0]], np.int32)
    ids, valid = R.decode_batch(off, cnt, 3, 3)
    assert valid.tolist() == [[1, 0, 0, 0]]
    assert ids[0].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]


def test_decode_batch_larger_row_wins():
    a, b = np.zeros((5, 7), bool), np.zeros((5, 7), bool)
    a[1:4, 1:5] = True
    b[2:5, 3:7] = True
    ca, cb = R.encode(a), R.encode(b)
    off = np.array([[0, len(ca), len(ca) + len(cb)]], np.int32)
    cnt = np.array([ca + cb], np.int32)
    ids, valid = R.decode_batch(off, cnt, 5, 7)
    assert valid.tolist() == [[1, 1]]
    assert np.array_equal(ids[0], np.where(b, 2, np.where(a, 1, 0)))


def test_encode_batch_layout():
    ids = np.array([[[1, 1, 0], [0, 2, 2], [3, 0, 2]]], np.int32)
    sel = np.array([[2, 0, 7, 1]], np.int32)
    ref = R.encode_batch(ids, sel, 9)
    # id 2: positions (x=1,y=1) = 4, (2,1) = 7, (2,2) = 8 -> [4,1,2,2];  id 7 is absent -> [9];  id 1: positions 0 and 3 -> [0,1,2,1,5]
    assert ref["offsets"].tolist() == [[0, 4, 4, 5, 10]]
    assert ref["counts"][0, :10].tolist() == [4, 1, 2, 2, 9, 0, 1, 2, 1, 5] and not ref["counts"][0, 10:].any()
    assert ref["area"].tolist() == [[3, 0, 0, 2]]
    assert bytes(ref["str_bytes"][0, :ref["str_offsets"][0, -1]]).decode() == "4121" + "9" + "01203"          # 2 - 1; 1 - 1, 5 - 2
    assert ref["str_offsets"].tolist() == [[0, 4, 4, 5, 10]]
    assert ref["counts"].shape == (1, 22) and ref["str_bytes"].shape == (1, 88)


def test_host_parser_rejects_garbage():
    _, to_c = _helpers()
    with pytest.raises(ValueError):
        to_c("41~")
    with pytest.raises(ValueError):
        to_c("PP")                                      # ends inside a count
