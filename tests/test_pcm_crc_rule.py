"""CPU: the rule and the surface of alac_hip_pcm_crc32.  alac_hip_crc32_combine (host only) against zlib.crc32 and, where zlib
cannot go, against the Python restatement of the header's identities (pcm_crc_ref.py), which is itself checked against zlib
here; the control values; the header, the binding table and the kernel's chunk sizes agree; calls without a GPU."""
import ctypes
import inspect
import os
import re
import zlib

import numpy as np

import alac_amd
from alac_amd import capi
import pcm_crc_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alac_hip_pcm_crc32_workspace_bytes", "alac_hip_pcm_crc32", "alac_hip_pcm_crc32_host", "alac_hip_crc32_combine"]
LENGTHS = [0, 1, 2, 3, 4, 15, 16, 17, 255, 4096, 2 ** 20 + 3]


def test_restatement_of_the_identities_equals_zlib():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 3, 4, 15, 16, 17, 255):
        for data in (rng.integers(0, 256, n, dtype=np.uint8).tobytes(), bytes(n)):
            assert cr.crc32_from_pure(cr.pure(data), n) == zlib.crc32(data)
            for cut in {0, n // 3, n}:
                a, b = data[:cut], data[cut:]
                assert cr.pure(data) == cr.mul(cr.pure(a), cr.x8_pow(len(b))) ^ cr.pure(b)
                assert cr.combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data)
    assert cr.x8_pow(0) == cr.ONE and cr.x8_pow(1) == cr.X8 == 0x00800000


def test_control_values():
    assert zlib.crc32(b"") == 0 and zlib.crc32(bytes(4)) == 0x2144df1c and zlib.crc32(bytes(8)) == 0x6522df69
    for n, want in ((0, 0), (4, 0x2144df1c), (8, 0x6522df69)):
        assert cr.crc32_from_pure(0, n) == want  # pure(zeros) is 0: the length term alone
        assert alac_amd.crc32_combine(0, want, n) == want
    # zeros appended to zeros: the combine carries the length
    assert alac_amd.crc32_combine(0x2144df1c, 0x2144df1c, 4) == 0x6522df69


def test_combine_equals_zlib_for_500_random_splits():
    rng = np.random.default_rng(2)
    lib = alac_amd.load_library()
    pieces = {}
    for n in LENGTHS:  # one random and one all-zero piece per length, hashed once
        pieces[n] = [rng.integers(0, 256, n, dtype=np.uint8).tobytes(), bytes(n)]
    seen_zero = 0
    for i in range(500):
        la, lb = (int(rng.choice(LENGTHS)) for _ in range(2))
        za, zb = (int(rng.integers(0, 2)) for _ in range(2))
        a, b = pieces[la][za], pieces[lb][zb]
        seen_zero += za and zb
        want = zlib.crc32(b, zlib.crc32(a))
        assert lib.alac_hip_crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == want, (la, lb, za, zb)
        assert alac_amd.crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == want
    assert seen_zero > 50
    # three pieces, joined left to right
    a, b, c = pieces[17][0], pieces[4096][0], pieces[255][0]
    ab = alac_amd.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b))
    assert alac_amd.crc32_combine(ab, zlib.crc32(c), len(c)) == zlib.crc32(a + b + c)


def test_combine_with_lengths_zlib_cannot_hash():
    rng = np.random.default_rng(3)
    for len_b in (2 ** 32, 2 ** 40, 2 ** 32 + 5, 2 ** 63 + 1):
        for _ in range(4):
            ca, cb = (int(x) for x in rng.integers(0, 2 ** 32, 2, dtype=np.uint64))
            assert alac_amd.crc32_combine(ca, cb, len_b) == cr.combine(ca, cb, len_b), len_b
    # 2^32 zero bytes behind nothing: crc32 of the zeros themselves, by the identity for crc32(A)
    z = cr.crc32_from_pure(0, 2 ** 32)
    assert alac_amd.crc32_combine(0, z, 2 ** 32) == z
    assert alac_amd.crc32_combine(zlib.crc32(b"abc"), z, 2 ** 32) == cr.crc32_from_pure(cr.mul(cr.pure(b"abc"), cr.x8_pow(2 ** 32)), 2 ** 32 + 3)


def test_library_exports_and_binds_the_calls():
    lib = ctypes.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES
    assert len(alac_amd.SIGNATURES["alac_hip_pcm_crc32"][1]) == 8
    assert len(alac_amd.SIGNATURES["alac_hip_pcm_crc32_host"][1]) == 6
    assert len(alac_amd.SIGNATURES["alac_hip_crc32_combine"][1]) == 3
    assert ctypes.sizeof(alac_amd.PcmDigest) == 16
    assert (alac_amd.PcmDigest.bytes.offset, alac_amd.PcmDigest.crc32.offset, alac_amd.PcmDigest.reserved.offset) == (0, 8, 12)


def test_workspace_bytes_without_a_gpu():
    lib = alac_amd.load_library()
    assert lib.alac_hip_pcm_crc32_workspace_bytes(0) == 0  # no ranges: nothing to hold (the call itself refuses 0)
    for n in (1, 2, 300, 1024, 2 ** 32 - 1):
        assert lib.alac_hip_pcm_crc32_workspace_bytes(n) >= n * 16


def test_calls_without_a_context_are_parameter_errors():
    lib = alac_amd.load_library()
    u64 = ctypes.c_uint64
    dig = (alac_amd.PcmDigest * 1)()
    assert lib.alac_hip_pcm_crc32(None, None, u64(0), None, 1, None, u64(0), dig) == -50
    assert lib.alac_hip_pcm_crc32_host(None, None, u64(0), None, 1, dig) == -50
    assert bytes(dig) == bytes(16)


def test_header_declares_the_calls_and_states_the_rule():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        text = f.read()
    flat = " ".join(text.split())
    for n in NAMES:
        assert n + "(" in flat, n
    for phrase in ("pure(A || B) = pure(A) * x^(8|B|) ^ pure(B)", "crc32(A) = pure(A) ^ 0xFFFFFFFF * x^(8|A|) ^ 0xFFFFFFFF",
                   "crc32(A || B) = crc32(A) * x^(8|B|) ^ crc32(B)", "0xEDB88320", "0x2144df1c", "0x6522df69",
                   "typedef struct alac_hip_pcm_digest", "uint64_t bytes;", "uint32_t crc32;", "uint32_t reserved;"):
        assert phrase in flat, phrase
    decl = flat[flat.index("int32_t alac_hip_pcm_crc32("):]
    decl = decl[:decl.index(";")]
    for arg in ("const void *d_pcm", "uint64_t total_bytes", "const uint64_t *h_ranges", "uint32_t num_ranges", "void *d_workspace",
                "uint64_t workspace_bytes", "alac_hip_pcm_digest *d_digests"):
        assert arg in decl, arg


def test_python_surface_and_chunk_constants():
    sig = inspect.signature(alac_amd.Context.pcm_crc32)
    assert list(sig.parameters) == ["self", "pcm", "ranges"] and sig.parameters["ranges"].default is None
    assert list(inspect.signature(alac_amd.crc32_combine).parameters) == ["crc_a", "crc_b", "len_b"]
    # the sizes the GPU tests take from the binding are those of the kernel's source
    with open(os.path.join(ROOT, "alac_amd", "csrc", "alac_kernels.hpp")) as f:
        hpp = f.read()
    with open(os.path.join(ROOT, "alac_amd", "csrc", "alac_pcm_crc.hip")) as f:
        hip = f.read()
    shift = int(re.search(r"kPcmCrcLaneShift = (\d+);", hpp).group(1))
    assert "kPcmCrcLaneBytes = 1u << kPcmCrcLaneShift;" in hpp and "kPcmCrcWaveBytes = 64 * kPcmCrcLaneBytes;" in hpp
    assert "kPcmCrcBlockBytes = 4 * kPcmCrcWaveBytes;" in hpp
    blocks = int(re.search(r"kPcmCrcMaxBlocks = (\d+);", hip).group(1))
    assert capi.PCM_CRC_LANE_BYTES == 1 << shift
    assert capi.PCM_CRC_WAVE_BYTES == 64 * capi.PCM_CRC_LANE_BYTES and capi.PCM_CRC_BLOCK_BYTES == 4 * capi.PCM_CRC_WAVE_BYTES
    assert capi.PCM_CRC_PASS_BYTES == blocks * capi.PCM_CRC_BLOCK_BYTES
