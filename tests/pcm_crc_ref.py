"""Python restatement of the identities of include/alac_hip.h (alac_hip_pcm_crc32): GF(2)[x] / P on reflected 32-bit words,
P = 0xEDB88320, bit 31 of a word is x^0.  Stands beside zlib.crc32 where zlib cannot go (lengths of 2^32 bytes and more)."""
POLY = 0xEDB88320
ONE = 0x80000000  # x^0
X8 = 0x00800000   # x^8


def mul(a, b):
    """a * b mod P"""
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def x8_pow(n):
    """x^(8n): square-and-multiply"""
    v, sq = ONE, X8
    while n:
        if n & 1:
            v = mul(v, sq)
        sq = mul(sq, sq)
        n >>= 1
    return v


def combine(crc_a, crc_b, len_b):
    """crc32(A || B) = crc32(A) * x^(8|B|) ^ crc32(B)"""
    return mul(crc_a, x8_pow(len_b)) ^ crc_b


def pure(data):
    """the register after data with initial value 0 and no final XOR, bit by bit"""
    r = 0
    for byte in data:
        r ^= byte
        for _ in range(8):
            r = (r >> 1) ^ (POLY if r & 1 else 0)
    return r


def crc32_from_pure(p, n):
    """crc32(A) = pure(A) ^ 0xFFFFFFFF * x^(8|A|) ^ 0xFFFFFFFF"""
    return p ^ mul(0xFFFFFFFF, x8_pow(n)) ^ 0xFFFFFFFF
