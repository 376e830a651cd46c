"""The join's hash (csrc/et_join.h) restated in Python integers, and its inverse: bodies that collide by construction, not by search.

  hash = mix(sum + mix(length * STEP + n_bytes)),  sum = term 0 + term 1 + ...,  term i = mix(word i + (i + 1) * STEP)

mix, the finaliser of splitmix64, is a bijection on 64 bits, and the sum is plain: given a wanted hash, a length, a byte count and all
words of a body but one FULL word (8 of its bytes belong to the body), the missing word follows by un-mixing -- solve_word.  Under
table_2bit (A = 00, C = 01, G = 10, T = 11, four symbols per byte, the first in the byte's top bits) every string of 8 k bytes is the
encoder's own body of a text of 32 k symbols, so whatever word comes out is a legitimate record -- text_2bit decodes it; a text shorter
by one symbol shares the body when that symbol is an A.  Plain integers, a module like bitwalk.py and limits.py, imported by name; it
knows nothing about the library.  tests/test_join_host.py holds hash_of against et_join_hash, tests/test_gpu_join.py the device against
both."""

M64 = (1 << 64) - 1
STEP = 0x9E3779B97F4A7C15  # ET_JOIN_STEP
_C1, _C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_I1, _I2 = pow(_C1, -1, 1 << 64), pow(_C2, -1, 1 << 64)


def mix(x):
    x ^= x >> 30
    x = (x * _C1) & M64
    x ^= x >> 27
    x = (x * _C2) & M64
    return x ^ (x >> 31)


def _unshift(y, s):
    """The x with x ^ (x >> s) == y, for s >= 22: the third term x >> 3 s is zero."""
    return y ^ (y >> s) ^ (y >> 2 * s)


def unmix(y):
    y = (_unshift(y, 31) * _I2) & M64
    y = (_unshift(y, 27) * _I1) & M64
    return _unshift(y, 30)


def term(i, word):
    return mix((word + (i + 1) * STEP) & M64)


def finish(total, n_bytes, length):
    return mix((total + mix((length * STEP + n_bytes) & M64)) & M64)


def words_of(body):
    """The body's 8-byte little-endian words, the last one zero-extended."""
    return [int.from_bytes(body[i : i + 8], "little") for i in range(0, len(body), 8)]


def body_of(words):
    """Full words back to back: a body of 8 * len(words) bytes."""
    return b"".join(w.to_bytes(8, "little") for w in words)


def hash_of(body, length):
    return finish(sum(term(i, w) for i, w in enumerate(words_of(bytes(body)))) & M64, len(body), length)


def solve_word(words_before, words_after, h, n_bytes, length):
    """The one full word that, between words_before and words_after, gives the body of n_bytes bytes under `length` the hash h."""
    i = len(words_before)
    assert 8 * (i + 1) <= n_bytes and (n_bytes + 7) // 8 == i + 1 + len(words_after), "the solved word is one of the body's full words"
    total = (unmix(h) - mix((length * STEP + n_bytes) & M64)) & M64
    rest = sum(term(j, w) for j, w in enumerate(words_before)) + sum(term(i + 1 + j, w) for j, w in enumerate(words_after))
    return (unmix((total - rest) & M64) - (i + 1) * STEP) & M64


def text_2bit(body, length):
    """The text of `length` symbols whose body under table_2bit is `body`: symbol q lies in bits 7 - 2 (q % 4), 6 - 2 (q % 4) of byte
    q // 4.  The callers assert that the encoder packs it back into `body`, which is what checks this bit order and the pad."""
    assert 4 * len(body) - 3 <= length <= 4 * len(body) if body else length == 0
    return bytes(b"ACGT"[(body[q // 4] >> (6 - 2 * (q % 4))) & 3] for q in range(length))
