"""The statement "gzip on the device" of include/dliom.h as an independent Python model -- sequential, a dictionary of last
occurrences, RFC 1951's tables written out -- and the case list of the gzip tests."""
import os
import random
import struct
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 4096
HEADER = bytes([0x1f, 0x8b, 0x08, 0, 0, 0, 0, 0, 0x04, 0x03])

# RFC 1951 section 3.2.5
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def bound(n):
    return 18 + n + 5 * max(1, -(-n // CHUNK))


class BitString:
    def __init__(self):
        self.bits = []

    def plain(self, value, n):  # an integer, least significant bit first
        self.bits += [(value >> k) & 1 for k in range(n)]

    def huffman(self, code, n):  # a Huffman code, most significant bit first
        self.bits += [(code >> (n - 1 - k)) & 1 for k in range(n)]

    def symbol(self, s):  # section 3.2.6
        if s < 144:
            self.huffman(0x30 + s, 8)
        elif s < 256:
            self.huffman(0x190 + s - 144, 9)
        elif s < 280:
            self.huffman(s - 256, 7)
        else:
            self.huffman(0xc0 + s - 280, 8)

    def to_bytes(self):
        bits = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(bits[8 * i + k] << k for k in range(8)) for i in range(len(bits) // 8))


def tokens_of(b):
    """[(position, length, distance)], distance 0 for a literal"""
    last, tokens, i, seen = {}, [], 0, 0
    n = len(b)
    while i < n:
        while seen < i:  # every position in front of i has been entered, token start or not
            if seen + 3 <= n:
                last[b[seen:seen + 3]] = seen
            seen += 1
        length, distance = 1, 0
        if i + 3 <= n and b[i:i + 3] in last:
            j = last[b[i:i + 3]]
            cap, l = min(258, n - i), 0
            while l < cap and b[j + l] == b[i + l]:
                l += 1
            if l >= 3:
                length, distance = l, i - j
        tokens.append((i, length, distance))
        i += length
    return tokens


def fixed_form(b, final):
    s = BitString()
    s.plain(0, 1)
    s.plain(1, 2)
    for at, length, distance in tokens_of(b):
        if distance == 0:
            s.symbol(b[at])
            continue
        code = 28 if length == 258 else max(k for k in range(28) if LENGTH_BASE[k] <= length)
        s.symbol(257 + code)
        s.plain(length - LENGTH_BASE[code], LENGTH_EXTRA[code])
        code = max(k for k in range(30) if DIST_BASE[k] <= distance)
        s.huffman(code, 5)
        s.plain(distance - DIST_BASE[code], DIST_EXTRA[code])
    s.symbol(256)
    s.plain(1 if final else 0, 1)
    s.plain(0, 2)
    return s.to_bytes() + b"\x00\x00\xff\xff"


def stored_form(b, final):
    return bytes([1 if final else 0]) + struct.pack("<HH", len(b), len(b) ^ 0xffff) + b


def chunk_form(b, final):
    """(bytes, stored?)"""
    stored = stored_form(b, final)
    if not b:
        return stored, True
    fixed = fixed_form(b, final)
    return (stored, True) if len(stored) < len(fixed) else (fixed, False)


def model(data, count=None):
    data = bytes(data)
    chunks = [data[i:i + CHUNK] for i in range(0, len(data), CHUNK)] or [b""]
    out = HEADER
    for k, chunk in enumerate(chunks):
        form, stored = chunk_form(chunk, k + 1 == len(chunks))
        if count is not None:
            count["chunks"] = count.get("chunks", 0) + 1
            count["chunks_stored"] = count.get("chunks_stored", 0) + (1 if stored else 0)
        out += form
    return out + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def model_cached(data, memo, count=None):
    """model(data, count), a chunk's form looked up in the dictionary `memo` under (chunk, final): for inputs of thousands
    of chunks out of a few distinct ones (big_segment)"""
    data = bytes(data)
    chunks = [data[i:i + CHUNK] for i in range(0, len(data), CHUNK)] or [b""]
    parts = [HEADER]
    for k, chunk in enumerate(chunks):
        key = (chunk, k + 1 == len(chunks))
        if key not in memo:
            memo[key] = chunk_form(*key)
        form, stored = memo[key]
        if count is not None:
            count["chunks"] = count.get("chunks", 0) + 1
            count["chunks_stored"] = count.get("chunks_stored", 0) + (1 if stored else 0)
        parts.append(form)
    parts.append(struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff))
    return b"".join(parts)


_chunk_kinds = None


def chunk_kinds():
    """six chunks of 4096 bytes: random bytes (stored form), zeros, random over 3 symbols, random over 2 symbols, b"ab"
    repeated, all byte values x 16"""
    global _chunk_kinds
    if _chunk_kinds is None:
        rng = random.Random(4096)
        _chunk_kinds = [rng.randbytes(CHUNK), bytes(CHUNK), bytes(rng.randrange(3) for _ in range(CHUNK)),
                        bytes(rng.randrange(2) for _ in range(CHUNK)), b"ab" * (CHUNK // 2), bytes(range(256)) * 16]
        assert all(len(c) == CHUNK for c in _chunk_kinds)
    return list(_chunk_kinds)


def big_segment(n, seed):
    """n bytes: the chunks of chunk_kinds() in a seeded random order, cut to n"""
    kinds, rng = chunk_kinds(), random.Random(seed)
    return b"".join(kinds[rng.randrange(len(kinds))] for _ in range(-(-n // CHUNK)))[:n]


def _with_match(length=None, distance=None):
    """bytes whose greedy parse holds a match of that length, or of that distance: random filler, a random pattern, filler,
    the pattern again, then a byte that ends the match (checked by the host test with token_lengths / token_distances)"""
    rng = random.Random(1000 * (length or 0) + (distance or 0))
    if length is None:
        length = 3
    if distance is None:
        distance = length + 7
    pattern, between = rng.randbytes(length), rng.randbytes(distance - length)
    follows = (between + pattern)[0]
    lead = rng.randbytes(11 if distance + length + 13 <= CHUNK else 0)  # the farthest ones start at the chunk's first byte
    return lead + pattern + between + pattern + bytes([follows ^ 0xff, 0x55])[:CHUNK - len(lead) - distance - length]


def _fixed_beats_stored_by(margin):
    """a short chunk whose fixed form is `margin` bytes below the stored one: n distinct 8-bit literals, k distinct 9-bit
    literals, then the first m bytes again (one match of length m at distance n + k).  Literals alone never get there:
    ceil((13 + 8 n + k) / 8) + 4 >= n + k + 6."""
    for n in range(3, 40):
        for m in range(3, 12):
            for k in range(4):
                data = bytes(range(n)) + bytes(range(144, 144 + k)) + bytes(range(m))
                form, stored = chunk_form(data, True)
                if not stored and len(stored_form(data, True)) - len(form) == margin:
                    return data
    raise AssertionError("no such chunk")


def cases():
    """[(name, bytes)]"""
    rng = random.Random(20261021)
    out = [("n=%d" % n, bytes(range(65, 65 + n))) for n in range(4)]
    out.append(("aaa", b"aaa"))
    out += [("run %d" % n, b"z" * n) for n in (258, 259, 260, 261)]
    out.append(("ab x 3000", b"ab" * 3000))
    far = bytes(4 + k % 250 for k in range(CHUNK))
    out.append(("distance 4093, cut at the chunk end", b"\x00\x01\x02" + far[3:4093] + b"\x00\x01\x02" + far[3:8] + b"\x09"))  # (the next chunk goes on as byte 3 does)
    out += [("%d zeros" % n, bytes(n)) for n in (4095, 4096, 4097, 12289)]
    straddle = bytes(4 + (k * 5) % 250 for k in range(CHUNK - 4)) + b"\x00\x01\x02\x03" + b"\x00\x01\x02\x03" + b"\x01\x02\x03\x00" * 3
    out.append(("a pattern across the chunk boundary", straddle))
    out.append(("all byte values x 3", bytes(range(256)) * 3))
    out += [("length %d" % n, _with_match(length=n)) for n in (3, 10, 11, 18, 19, 34, 35, 66, 67, 130, 131, 257, 258)]
    # (inside a chunk of 4096 a distance is at most 4093: the codes' boundaries up to there, and 4093 itself)
    boundaries = sorted(set(d for b in DIST_BASE if b <= 4093 for d in (b - 1, b) if d >= 1) | {4093})
    out += [("distance %d" % d, _with_match(distance=d)) for d in boundaries if d >= 3]
    out += [("distance 1", b"\x07" * 9), ("distance 2", b"\x07\x08" * 4)]
    out.append(("10000 random bytes", rng.randbytes(10000)))
    out.append(("fixed wins by a byte", _fixed_beats_stored_by(1)))
    out.append(("fixed ties with stored", _fixed_beats_stored_by(0)))
    for k in range(200):
        symbols = (2, 3, 256)[k % 3]
        n = (CHUNK, 2 * CHUNK)[(k // 3) % 2] + rng.randrange(-40, 41)
        out.append(("random %d: %d symbols, %d bytes" % (k, symbols, n), bytes(rng.randrange(symbols) for _ in range(n))))
    return out


def token_lengths(data):
    return {t[1] for i in range(0, len(data), CHUNK) for t in tokens_of(data[i:i + CHUNK]) if t[2]}


def token_distances(data):
    return {t[2] for i in range(0, len(data), CHUNK) for t in tokens_of(data[i:i + CHUNK]) if t[2]}
