"""The tables and code bits of d-liom_amd/csrc/gzip_format.h, which the kernels of gzip.hip and the host encoder share,
against arithmetic written here: polynomials over GF(2) modulo 0x104C11DB7 on Python integers, zlib's CRC-32, and the
bit strings of tests/gzip_common.py from RFC 1951's tables.  The encoders reach only a part of them on small inputs: a
chunk of 4096 bytes never emits a distance above 4093, the host encoder computes its CRC bytewise, and pow2[k] is read
only by a segment of at least 2^k bytes.  Here every entry is compared: byte[256], shift16[256], pow2[32],
fixed_symbol(0..285), match_bits over every length at every distance code's two ends and over every distance 1..32768.

tests/cpp/gzip_format_check.cc prints them; it is built with g++ and once more, stand-alone, with
-fsanitize=address,undefined.  No GPU.  Plus model_cached of gzip_common.py against model."""
import os
import random
import subprocess
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gzip_common as gz  # noqa: E402

CHECK = os.path.join(gz.ROOT, "tests", "cpp", "gzip_format_check.cc")
DISTANCES = sorted({d for b in gz.DIST_BASE for d in (b - 1, b) if d >= 1} | {32768})
POLY = 0x104C11DB7  # x^32 + x^26 + ... + 1, bit k the coefficient of x^k
M32 = 0xffffffff


# ---- polynomials over GF(2), natural bit order ----
def reflect(w):
    """a word of the header (bit 31 the coefficient of x^0) <-> the polynomial as an integer (bit k that of x^k)"""
    return int("{:032b}".format(w)[::-1], 2)


def poly_mod(a):
    while a.bit_length() > 32:
        a ^= POLY << (a.bit_length() - 33)
    return a


def poly_mul(a, b):
    p = 0
    while b:
        if b & 1:
            p ^= a
        a <<= 1
        b >>= 1
    return poly_mod(p)


def x_to_the(e):
    """x^e mod P by square and multiply"""
    result, square = 1, 2
    while e:
        if e & 1:
            result = poly_mul(result, square)
        square = poly_mul(square, square)
        e >>= 1
    return result


def mul_words(a, b):
    return reflect(poly_mul(reflect(a), reflect(b)))


# ---- the program's output ----
def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, CHECK])
    return subprocess.check_output([exe] + [str(d) for d in DISTANCES]).decode()


def parse(text):
    out = {"m": {}, "mul": []}
    for line in text.splitlines():
        f = line.split()
        if f[0] in ("byte", "shift16", "pow2"):
            out[f[0]] = [int(v, 16) for v in f[1:]]
        elif f[0] == "sym":
            out["sym"] = [(int(f[1 + 2 * s], 16), int(f[2 + 2 * s])) for s in range((len(f) - 1) // 2)]
        elif f[0] == "m":
            out["m"][(int(f[1]), int(f[2]))] = (int(f[3], 16), int(f[4]))
        elif f[0] == "mul":
            out["mul"].append(tuple(int(v, 16) for v in f[1:]))
        else:
            raise AssertionError("unknown line: " + line[:60])
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("gzip_format"), "gzip_format_check", ["-O2"])


@pytest.fixture(scope="module")
def tables(printed):
    return parse(printed)


def test_sanitized_build_prints_the_same(tmp_path, printed):
    """the stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer: no shift by 32 or more, no index
    outside a table, for any length or distance"""
    text = _build_and_run(tmp_path, "gzip_format_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert text == printed


def test_everything_asked_for_is_printed(tables):
    assert [len(tables[k]) for k in ("byte", "shift16", "pow2", "sym")] == [256, 256, 32, 286]
    want = {(l, d) for l in range(3, 259) for d in DISTANCES} | {(l, d) for l in (3, 258) for d in range(1, 32769)}
    assert set(tables["m"]) == want and len(tables["mul"]) == 400
    assert 24576 in DISTANCES and 24577 in DISTANCES and 4 in DISTANCES and 5 in DISTANCES and len(DISTANCES) == 5 + 2 * 25 + 1


def test_powers_of_x(tables):
    for k in range(32):
        assert tables["pow2"][k] == reflect(x_to_the(8 * 2 ** k)), k
    for m in range(256):
        assert tables["shift16"][m] == reflect(x_to_the(128 * m)), m
    assert len(set(tables["pow2"])) == 32  # (the order of x modulo P is 2^32 - 1: no two of them are equal)


def test_crc_mul_is_the_product(tables):
    for a, b, p in tables["mul"]:
        assert p == mul_words(a, b), (hex(a), hex(b))
    assert tables["mul"][1][2] == tables["mul"][1][1] and tables["mul"][0][2] == 0  # x^0 * b = b, 0 * b = 0


def test_tables_against_zlib(tables):
    for b in range(256):
        # one byte c from the register 0xffffffff: byte[c ^ 0xff] ^ 0x00ffffff, complemented
        assert tables["byte"][b] == zlib.crc32(bytes([b ^ 0xff])) ^ 0xff000000, b
    rng = random.Random(7)
    for message in (b"", b"a", b"123456789", rng.randbytes(77)):
        register = zlib.crc32(message) ^ M32
        for k in range(25):
            assert zlib.crc32(message + bytes(1 << k)) == mul_words(register, tables["pow2"][k]) ^ M32, (message[:9], k)
        for m in (1, 2, 17, 255):
            assert zlib.crc32(message + bytes(16 * m)) == mul_words(register, tables["shift16"][m]) ^ M32, (message[:9], m)


def value_of(s):
    return sum(bit << k for k, bit in enumerate(s.bits)), len(s.bits)


def test_fixed_symbols(tables):
    for symbol in range(286):
        s = gz.BitString()
        s.symbol(symbol)
        assert tables["sym"][symbol] == value_of(s), symbol


def test_match_bits(tables):
    """length symbol, its extra bits, the distance code, its extra bits: as gzip_common.fixed_form strings them"""
    length_part, distance_part = {}, {}
    for length in range(3, 259):
        code = 28 if length == 258 else max(k for k in range(28) if gz.LENGTH_BASE[k] <= length)
        s = gz.BitString()
        s.symbol(257 + code)
        s.plain(length - gz.LENGTH_BASE[code], gz.LENGTH_EXTRA[code])
        assert length - gz.LENGTH_BASE[code] < 1 << gz.LENGTH_EXTRA[code] or length == 258
        length_part[length] = list(s.bits)
    for distance in range(1, 32769):
        code = max(k for k in range(30) if gz.DIST_BASE[k] <= distance)
        s = gz.BitString()
        s.huffman(code, 5)
        s.plain(distance - gz.DIST_BASE[code], gz.DIST_EXTRA[code])
        assert distance - gz.DIST_BASE[code] < 1 << gz.DIST_EXTRA[code]
        distance_part[distance] = list(s.bits)
    wrong, longest = [], 0
    for (length, distance), got in tables["m"].items():
        s = gz.BitString()
        s.bits = length_part[length] + distance_part[distance]
        if got != value_of(s):
            wrong.append((length, distance, got, value_of(s)))
        longest = max(longest, got[1])
    assert not wrong, (len(wrong), wrong[:8])
    assert longest == 31 and tables["m"][(257, 32768)][1] == 31  # 8 + 5 + 5 + 13: never more than a word holds


def test_model_cached_equals_model():
    kinds = gz.chunk_kinds()
    assert len(kinds) == 6 and all(len(c) == gz.CHUNK for c in kinds) and len(set(kinds)) == 6
    assert [gz.chunk_form(c, False)[1] for c in kinds] == [True, False, False, False, False, False]
    memo = {}
    inputs = [b"", kinds[2][:1], kinds[1] + kinds[1] + kinds[1][:5], kinds[0] + kinds[4] + kinds[0] + kinds[4] + kinds[4][:4095],
              kinds[3] * 3, gz.big_segment(9 * gz.CHUNK + 37, 1), gz.big_segment(9 * gz.CHUNK + 37, 2), gz.big_segment(2 * gz.CHUNK, 1)]
    for data in inputs:
        count, cached_count = {}, {}
        want = gz.model(data, count)
        assert gz.model_cached(data, memo, cached_count) == want and cached_count == count, len(data)
        assert gz.model_cached(data, memo) == want and zlib.decompress(want, 31) == data  # (every form out of the dictionary now)
    # a chunk as the last and as an inner one are two entries; the short last chunks are entries of their own
    assert (kinds[3], True) in memo and (kinds[3], False) in memo and (kinds[4][:4095], True) in memo
    assert gz.big_segment(9 * gz.CHUNK + 37, 1) != gz.big_segment(9 * gz.CHUNK + 37, 2)
    assert gz.big_segment(5000, 3) == gz.big_segment(9000, 3)[:5000] and len(gz.big_segment(0, 1)) == 0
