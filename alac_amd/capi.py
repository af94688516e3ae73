"""ctypes binding of libalac_hip.so (the C-ABI declared in include/alac_hip.h).

PyTorch is used only as the owner of device memory and streams: every call below hands raw device
pointers to the HIP library.  There is no CPU fallback: if the library or a GPU is missing the
import of the library / creation of a context raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ALAC_HIP_LIB") or os.path.join(_HERE, "libalac_hip.so")  # ALAC_HIP_LIB: A/B runs against another build
SYNTH_PATH = os.path.join(_HERE, "libalac_synth.so")

STATE_INT16 = 64
BPS = {16: 2, 20: 3, 24: 3, 32: 4}


class Format(C.Structure):
    _fields_ = [("frame_size", C.c_uint32), ("bit_depth", C.c_uint32), ("num_channels", C.c_uint32),
                ("sample_rate", C.c_uint32)]

    @property
    def bytes_per_frame(self):
        return self.num_channels * BPS[self.bit_depth]

    @property
    def packet_bytes(self):
        return self.frame_size * self.bytes_per_frame


DITHER_NONE, DITHER_TPDF = 0, 1


class Dither(C.Structure):
    """alac_hip_dither"""
    _fields_ = [("mode", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64)]


class IntSource(C.Structure):
    """alac_hip_int_source: the containers of an integer source, their significant bits and their strides (in containers)"""
    _fields_ = [("container_bytes", C.c_uint32), ("bits", C.c_uint32), ("left_justified", C.c_uint32),
                ("reserved", C.c_uint32), ("channel_stride", C.c_uint64), ("frame_stride", C.c_uint64)]


class FloatReport(C.Structure):
    """alac_hip_float_report: one per segment of alac_hip_float_probe, 32 bytes"""
    _fields_ = [("over_range", C.c_uint64), ("nan", C.c_uint64), ("need_bits", C.c_uint32), ("peak_bits", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


class IntReport(C.Structure):
    """alac_hip_int_report: one per segment of alac_hip_int_probe, 32 bytes"""
    _fields_ = [("out_of_range", C.c_uint64), ("differing_frames", C.c_uint64), ("need_bits", C.c_uint32), ("peak", C.c_uint32),
                ("pad_bits", C.c_uint32), ("reserved", C.c_uint32)]


class PcmDigest(C.Structure):
    """alac_hip_pcm_digest: one per range of alac_hip_pcm_crc32, 16 bytes"""
    _fields_ = [("bytes", C.c_uint64), ("crc32", C.c_uint32), ("reserved", C.c_uint32)]


class LoudnessReport(C.Structure):
    """alac_hip_loudness_report: one per segment of alac_hip_loudness_int / _float, 32 bytes"""
    _fields_ = [("first_block", C.c_uint32), ("num_blocks", C.c_uint32), ("peak", C.c_double), ("nonfinite", C.c_uint64),
                ("reserved", C.c_uint64)]


class TruePeakReport(C.Structure):
    """alac_hip_true_peak_report: one per segment of alac_hip_true_peak_int / _float, 32 bytes"""
    _fields_ = [("true_peak", C.c_double), ("peak", C.c_double), ("nonfinite", C.c_uint64), ("reserved", C.c_uint64)]


class ResampleReport(C.Structure):
    """alac_hip_resample_report: one per segment of alac_hip_resample_int / _float, 32 bytes"""
    _fields_ = [("out_first", C.c_uint64), ("out_frames", C.c_uint64), ("peak", C.c_double), ("nonfinite", C.c_uint64)]


# the output frames of a block's tile of k_resample at the usual ratios (kResampleTile, alac_kernels.hpp; long filters take
# fewer, resample_tile()): the size at which the kernel changes path, for the tests
RESAMPLE_TILE = 512

# the frames of a lane's run of k_true_peak by oversampling factor (true_peak_run, alac_kernels.hpp); a block covers 256 runs:
# the sizes at which the kernel changes path, for the tests
TRUE_PEAK_RUN = {4: 53, 2: 105, 1: 64}
TRUE_PEAK_BLOCK_RUNS = 256

# what a lane, a wave, a block and one pass of the whole grid of k_pcm_crc take (alac_kernels.hpp, alac_pcm_crc.hip): the sizes
# at which the kernel changes path, for the tests
PCM_CRC_LANE_BYTES = 64
PCM_CRC_WAVE_BYTES = 64 * PCM_CRC_LANE_BYTES
PCM_CRC_BLOCK_BYTES = 4 * PCM_CRC_WAVE_BYTES
PCM_CRC_PASS_BYTES = 1024 * PCM_CRC_BLOCK_BYTES


def make_format(frame_size=4096, bit_depth=16, num_channels=2, sample_rate=44100):
    return Format(frame_size, bit_depth, num_channels, sample_rate)


_vp, _u32, _i32, _u64 = C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64

# name -> (restype, argtypes); mirrors include/alac_hip.h one to one
SIGNATURES = {
    "alac_hip_device_count": (_i32, []),
    "alac_hip_create": (_i32, [C.POINTER(_vp), _i32, _vp]),
    "alac_hip_destroy": (None, [_vp]),
    "alac_hip_synchronize": (_i32, [_vp]),
    "alac_hip_last_error": (C.c_char_p, [_vp]),
    "alac_hip_encode_regime": (C.c_char_p, [_vp, C.POINTER(Format), _u32]),
    "alac_hip_debug_waves_offset": (_u64, [C.POINTER(Format), _u32, _u32]),
    "alac_hip_set_option": (_i32, [_vp, C.c_char_p, _i32]),
    "alac_hip_get_option": (_i32, [_vp, C.c_char_p, C.POINTER(_i32)]),
    "alac_hip_stream": (_vp, [_vp]),
    "alac_hip_encode_workspace_bytes": (_u64, [C.POINTER(Format), _u32, _u32]),
    "alac_hip_encode_max_output_bytes": (_u64, [C.POINTER(Format), _u32]),
    "alac_hip_encode": (_i32, [_vp, C.POINTER(Format), _vp, _vp, _u32, _vp, _u32, _vp, _i32, _vp, _u64,
                               _vp, _u64, _vp, _vp]),
    "alac_hip_encode_segmented": (_i32, [_vp, C.POINTER(Format), _vp, _vp, _u32, _vp, _u32, _u32, _vp, _i32, _vp, _u64,
                                         _vp, _u64, _vp, _vp]),
    "alac_hip_encode_float_workspace_bytes": (_u64, [C.POINTER(Format), _u32, _u32]),
    "alac_hip_encode_float": (_i32, [_vp, C.POINTER(Format), _vp, _u64, _u64, _vp, _u32, _vp, _u32, _u32, _vp, _i32, _vp, _u64,
                                     _vp, _u64, _vp, _vp, _vp]),
    "alac_hip_encode_float_host": (_i32, [_vp, C.POINTER(Format), _vp, _u64, _u64, _vp, _u32, _vp, _u32, _vp, _i32, _vp, _u64,
                                          _vp, C.POINTER(_u64), _vp]),
    "alac_hip_encode_float_dither": (_i32, [_vp, C.POINTER(Format), _vp, _u64, _u64, _vp, _u32, _vp, _u32, _u32, _vp, _i32, _vp,
                                            _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "alac_hip_encode_float_dither_host": (_i32, [_vp, C.POINTER(Format), _vp, _u64, _u64, _vp, _u32, _vp, _u32, _vp, _i32, _vp,
                                                 _u64, _vp, C.POINTER(_u64), _vp, _vp, _vp]),
    "alac_hip_pcm_requantize": (_i32, [_vp, C.POINTER(Format), _vp, _vp, _vp, _u32, _vp, _u64, _vp, _vp, _vp]),
    "alac_hip_pcm_requantize_host": (_i32, [_vp, C.POINTER(Format), _vp, _vp, _vp, _u32, _vp, _u64, _vp, _vp, _vp]),
    "alac_hip_encode_int_workspace_bytes": (_u64, [C.POINTER(Format), _u32, _u32]),
    "alac_hip_encode_int": (_i32, [_vp, C.POINTER(Format), _vp, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _i32, _vp, _u64, _vp, _u64,
                                   _vp, _vp, _vp, _vp, _vp]),
    "alac_hip_encode_int_host": (_i32, [_vp, C.POINTER(Format), _vp, _vp, _vp, _u32, _vp, _u32, _vp, _i32, _vp, _u64, _vp,
                                        C.POINTER(_u64), _vp, _vp, _vp]),
    "alac_hip_profile_begin": (_i32, [_vp, _u32]),
    "alac_hip_profile_end": (_i32, [_vp, C.POINTER(_u32), C.POINTER(C.c_float), C.POINTER(_u32)]),
    "alac_hip_num_stages": (_u32, []),
    "alac_hip_stage_name": (C.c_char_p, [_u32]),
    "alac_hip_magic_cookie": (_u32, [C.POINTER(Format), _u32, _u32, _vp]),
    "alac_hip_magic_cookie_size": (_u32, [C.POINTER(Format)]),
    "alac_hip_magic_cookie_full": (_u32, [C.POINTER(Format), _u32, _u32, _vp, _u32]),
    "alac_hip_state_int16": (_u32, [C.POINTER(Format)]),
    "alac_hip_decode_workspace_bytes": (_u64, [C.POINTER(Format), _u32]),
    "alac_hip_decode_workspace_bytes_stream": (_u64, [C.POINTER(Format), _u32, _u64]),
    "alac_hip_decode": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _vp, _vp]),
    "alac_hip_format_from_cookie": (_i32, [_vp, _u32, C.POINTER(Format)]),
    "alac_hip_pc_block": (_i32, [_vp, _vp, _vp, _u32, _u32, _i32, _vp, _i32, _u32, _u32]),
    "alac_hip_unpc_block": (_i32, [_vp, _vp, _vp, _u32, _u32, _i32, _vp, _i32, _u32, _u32]),
    "alac_hip_dyn_comp": (_i32, [_vp, _u32, _u32, _u32, _vp, _u32, _u32, _i32, _i32, _vp, _u32, _vp]),
    "alac_hip_dyn_decomp": (_i32, [_vp, _u32, _u32, _u32, _vp, _u32, _u32, _vp, _u32, _i32, _i32, _vp, _vp]),
    "alac_hip_encode_host": (_i32, [_vp, C.POINTER(Format), _vp, _u64, _u32, _vp, _i32, _vp, _u64, _vp,
                                    C.POINTER(_u64)]),
    "alac_hip_encode_host_segments": (_i32, [_vp, C.POINTER(Format), _vp, _vp, _u32, _vp, _u32, _vp, _i32, _vp, _u64, _vp,
                                             C.POINTER(_u64)]),
    "alac_hip_decode_host": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    "alac_hip_decode_float": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _u64, _vp, _vp]),
    "alac_hip_decode_float_host": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _vp]),
    "alac_hip_decode_int": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _vp, _vp, _vp, _vp]),
    "alac_hip_decode_int_host": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "alac_hip_verify_workspace_bytes_stream": (_u64, [C.POINTER(Format), _u32, _u64]),
    "alac_hip_verify": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "alac_hip_verify_host": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "alac_hip_verify_float": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "alac_hip_verify_float_host": (_i32, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "alac_hip_float_probe_workspace_bytes": (_u64, [_u32]),
    "alac_hip_float_probe": (_i32, [_vp, _vp, _u32, _u64, _u64, _u64, _vp, _u32, _vp, _u64, _vp]),
    "alac_hip_float_probe_host": (_i32, [_vp, _vp, _u32, _u64, _u64, _u64, _vp, _u32, _vp]),
    "alac_hip_float_report_depth": (_u32, [_vp]),
    "alac_hip_int_probe_workspace_bytes": (_u64, [_u32]),
    "alac_hip_int_probe": (_i32, [_vp, _vp, _vp, _u32, _u64, _vp, _u32, _vp, _u64, _vp]),
    "alac_hip_int_probe_host": (_i32, [_vp, _vp, _vp, _u32, _u64, _vp, _u32, _vp]),
    "alac_hip_int_report_depth": (_u32, [_vp]),
    "alac_hip_pcm_crc32_workspace_bytes": (_u64, [_u32]),
    "alac_hip_pcm_crc32": (_i32, [_vp, _vp, _u64, _vp, _u32, _vp, _u64, _vp]),
    "alac_hip_pcm_crc32_host": (_i32, [_vp, _vp, _u64, _vp, _u32, _vp]),
    "alac_hip_crc32_combine": (_u32, [_u32, _u32, _u64]),
    "alac_hip_loudness_workspace_bytes": (_u64, [_u32, _u32, _u64, _u32]),
    "alac_hip_loudness_int": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _vp, _u32, _vp, _u64, _vp, _u64, _vp]),
    "alac_hip_loudness_float": (_i32, [_vp, _vp, _u32, _u64, _u64, _u32, _u64, _vp, _u32, _vp, _u64, _vp, _u64, _vp]),
    "alac_hip_loudness_int_host": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _vp, _u32, _vp, _u64, _vp]),
    "alac_hip_loudness_float_host": (_i32, [_vp, _vp, _u32, _u64, _u64, _u32, _u64, _vp, _u32, _vp, _u64, _vp]),
    "alac_hip_loudness_filter": (_i32, [_u32, _vp]),
    "alac_hip_loudness_rows": (_u64, [_u32, _u64, _vp, _u32]),
    "alac_hip_loudness_integrated": (_i32, [_vp, _u64, _u32, _u32, _vp, C.POINTER(C.c_double)]),
    "alac_hip_true_peak_workspace_bytes": (_u64, [_u32, _u32]),
    "alac_hip_true_peak_int": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _vp, _u32, _vp, _u64, _vp, _vp]),
    "alac_hip_true_peak_float": (_i32, [_vp, _vp, _u32, _u64, _u64, _u32, _u64, _vp, _u32, _vp, _u64, _vp, _vp]),
    "alac_hip_true_peak_int_host": (_i32, [_vp, _vp, _vp, _u32, _u32, _u64, _vp, _u32, _vp, _vp]),
    "alac_hip_true_peak_float_host": (_i32, [_vp, _vp, _u32, _u64, _u64, _u32, _u64, _vp, _u32, _vp, _vp]),
    "alac_hip_true_peak_filter": (_i32, [_u32, C.POINTER(_u32), C.POINTER(_u32), _vp]),
    "alac_hip_resample_filter": (_i32, [_u32, _u32, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), _vp]),
    "alac_hip_resample_frames": (_u64, [_u32, _u32, _u64, _vp, _u32, _vp]),
    "alac_hip_resample_workspace_bytes": (_u64, [_u32, _u32, _u32, _u32]),
    "alac_hip_resample_int": (_i32, [_vp, _vp, _vp, _u32, _u32, _u32, _u64, _vp, _u32, _vp, _u64, _vp, _u64, _u64, _vp]),
    "alac_hip_resample_float": (_i32, [_vp, _vp, _u32, _u64, _u64, _u32, _u32, _u64, _vp, _u32, _vp, _u64, _vp, _u64, _u64,
                                       _vp]),
    "alac_hip_resample_int_host": (_i32, [_vp, _vp, _vp, _u32, _u32, _u32, _u64, _vp, _u32, _vp, _u64, _u64, _vp]),
    "alac_hip_resample_float_host": (_i32, [_vp, _vp, _u32, _u64, _u64, _u32, _u32, _u64, _vp, _u32, _vp, _u64, _u64, _vp]),
    "alac_synth_frame": (None, [_u64, _u32, _u32, _u32, _vp]),
    "alac_synth_pcm": (None, [_u64, _u32, _u32, _u32, _u32, _vp]),
    "alac_hip_synth_pcm": (_i32, [_vp, _u64, _u32, C.POINTER(Format), _vp]),
    "alac_hip_shard_range": (_i32, [_u64, _u32, _u32, C.POINTER(_u64), C.POINTER(_u64)]),
    "alac_hip_shard_offsets": (_i32, [_vp, _u32, _vp]),
    "alac_hip_comm_unique_id": (_i32, [_vp]),
    "alac_hip_comm_create": (_i32, [C.POINTER(_vp), _i32, _vp, _u32, _u32]),
    "alac_hip_comm_destroy": (None, [_vp]),
    "alac_hip_comm_rank": (_u32, [_vp]),
    "alac_hip_comm_world": (_u32, [_vp]),
    "alac_hip_comm_last_error": (C.c_char_p, [_vp]),
    "alac_hip_reassemble_begin": (_i32, [_vp, _u32, _vp, _u64, _u64, _vp, _u32, _vp, _vp]),
    "alac_hip_reassemble_finish": (_i32, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "alac_hip_reassemble": (_i32, [_vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _u64, _vp, _vp]),
}

COMM_ID_BYTES = 128
COMM_SLOTS = 4

_lib = None


def load_library(path=None):
    """dlopen libalac_hip.so and bind every symbol of include/alac_hip.h (raises if one is missing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise FileNotFoundError(
            f"{p} is missing: build it with `make -C alac_amd/csrc` (or __graft_entry__.build()); "
            "the HIP path has no CPU fallback")
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def source_fingerprint():
    """sha256 (first 16 hex digits) over the kernel and C-ABI sources under alac_amd/csrc + include/: what a set of PMC
    counters under profiles/ was collected on (bench.py refuses counters of other sources; no GPU or library needed)"""
    import hashlib
    h = hashlib.sha256()
    root = os.path.dirname(_HERE)
    files = []
    for d in (os.path.join(_HERE, "csrc"), os.path.join(root, "include")):
        for dp, _, fn in os.walk(d):
            files += [os.path.join(dp, f) for f in fn if f.endswith((".hip", ".hpp", ".h", ".cpp", ".c"))]
    for f in sorted(files):
        h.update(os.path.relpath(f, root).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def shard_range(num_units, world, rank):
    """(first, count) of the units rank `rank` of `world` encodes (alac_hip_shard_range); raises on bad arguments"""
    first, count = _u64(), _u64()
    if load_library().alac_hip_shard_range(num_units, world, rank, C.byref(first), C.byref(count)) != 0:
        raise ValueError(f"bad shard arguments: world {world}, rank {rank}")
    return first.value, count.value


def shard_offsets(shard_bytes):
    """byte offsets of the shards in the re-assembled stream, [world + 1] (alac_hip_shard_offsets)"""
    n = len(shard_bytes)
    src = (_u64 * n)(*[int(x) for x in shard_bytes])
    dst = (_u64 * (n + 1))()
    if load_library().alac_hip_shard_offsets(src, n, dst) != 0:
        raise ValueError("bad shard sizes")
    return list(dst)


def crc32_combine(crc_a, crc_b, len_b):
    """zlib.crc32(A + B) from crc_a = zlib.crc32(A), crc_b = zlib.crc32(B) and len_b = len(B) (alac_hip_crc32_combine):
    host only, no GPU needed"""
    return int(load_library().alac_hip_crc32_combine(int(crc_a) & 0xFFFFFFFF, int(crc_b) & 0xFFFFFFFF, int(len_b)))


def loudness_filter(sample_rate):
    """alac_hip_loudness_filter: the K-weighting biquads of a sample rate as a float64 array {b0, b1, b2, a1, a2} of the
    shelf, then of the high-pass.  Host only, no GPU needed."""
    out = np.zeros(10, dtype=np.float64)
    if load_library().alac_hip_loudness_filter(int(sample_rate), out.ctypes.data) != 0:
        raise ValueError("loudness_filter: the sample rate must be a multiple of 10 in [8000, 384000]")
    return out


def loudness_rows(sample_rate, total_frames, seg_first_frame=None):
    """alac_hip_loudness_rows: the 100 ms rows the segments of a table have in all.  Host only."""
    table = None if seg_first_frame is None else np.ascontiguousarray(seg_first_frame, dtype=np.uint64)
    return int(load_library().alac_hip_loudness_rows(int(sample_rate), int(total_frames),
                                                     None if table is None else table.ctypes.data,
                                                     1 if table is None else table.size - 1))


def integrated_loudness(energy, hop, weights=None):
    """alac_hip_loudness_integrated: the gated BS.1770 loudness in LUFS of the rows [blocks, channels] of ONE segment
    (float64; hop = sample_rate // 10); weights None: BS.1770's in the ALAC channel order.  -inf where no block passes the
    gates.  Host only, no GPU needed."""
    e = np.ascontiguousarray(energy, dtype=np.float64)
    if e.ndim != 2 or not 1 <= e.shape[1] <= 8:
        raise ValueError("integrated_loudness: energy must be [blocks, channels] with 1..8 channels")
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    if w is not None and w.shape != (e.shape[1],):
        raise ValueError("integrated_loudness: one weight per channel")
    out = C.c_double(0.0)
    rc = load_library().alac_hip_loudness_integrated(e.ctypes.data if e.size else None, e.shape[0], e.shape[1], int(hop),
                                                     None if w is None else w.ctypes.data, C.byref(out))
    if rc != 0:
        raise ValueError("integrated_loudness: bad arguments")
    return out.value


def true_peak_filter(sample_rate):
    """alac_hip_true_peak_filter: (factor, coefficients) of a sample rate: the oversampling factor F (4, 2 or 1) and the
    phases 1 .. F-1 of the interpolator as a float64 array [F - 1, taps] (taps 12, 24, or 0 where F is 1).  Host only, no GPU
    needed."""
    factor, taps = _u32(0), _u32(0)
    out = np.zeros(36, dtype=np.float64)
    if load_library().alac_hip_true_peak_filter(int(sample_rate), C.byref(factor), C.byref(taps), out.ctypes.data) != 0:
        raise ValueError("true_peak_filter: the sample rate must be a multiple of 10 in [8000, 384000]")
    n = (factor.value - 1) * taps.value
    return factor.value, out[:n].reshape(factor.value - 1, taps.value).copy()


def resample_filter(in_rate, out_rate):
    """alac_hip_resample_filter: (L, M, coefficients) of a rate pair: out_rate / gcd, in_rate / gcd and the polyphase filter
    h_p[k] as a float64 array [L, K].  Host only, no GPU needed."""
    lib = load_library()
    L, M, K = _u32(0), _u32(0), _u32(0)
    if lib.alac_hip_resample_filter(int(in_rate), int(out_rate), C.byref(L), C.byref(M), C.byref(K), None) != 0:
        raise ValueError("resample_filter: the rates must be different multiples of 10 in [8000, 384000] with L and M of at "
                         "most 640")
    out = np.zeros((L.value, K.value), dtype=np.float64)
    if lib.alac_hip_resample_filter(int(in_rate), int(out_rate), C.byref(L), C.byref(M), C.byref(K), out.ctypes.data) != 0:
        raise ValueError("resample_filter: bad arguments")
    return L.value, M.value, out


def resample_frames(in_rate, out_rate, total_frames, seg_first_frame=None):
    """alac_hip_resample_frames: (total, out_first): the output frames of all segments back to back and every segment's
    first output frame, a uint64 array [num_segments + 1].  (0, zeros) for arguments the calls refuse.  Host only."""
    table = None if seg_first_frame is None else np.ascontiguousarray(seg_first_frame, dtype=np.uint64)
    nseg = 1 if table is None else max(0, table.size - 1)
    out_first = np.zeros(nseg + 1, dtype=np.uint64)
    total = int(load_library().alac_hip_resample_frames(int(in_rate), int(out_rate), int(total_frames),
                                                        None if table is None else table.ctypes.data, nseg,
                                                        out_first.ctypes.data))
    return total, out_first


def synth_pcm(first_frame, num_frames, fmt):
    """Deterministic synthetic PCM (alac_synth.c) as a uint8 numpy array, host side, no GPU needed."""
    p = SYNTH_PATH if os.path.exists(SYNTH_PATH) else LIB_PATH
    if not os.path.exists(p):
        raise FileNotFoundError(f"{SYNTH_PATH} missing: run `make -C alac_amd/csrc`")
    lib = C.CDLL(p)
    lib.alac_synth_pcm.argtypes = SIGNATURES["alac_synth_pcm"][1]
    lib.alac_synth_pcm.restype = None
    out = np.zeros(num_frames * fmt.packet_bytes, dtype=np.uint8)
    lib.alac_synth_pcm(first_frame, num_frames, fmt.frame_size, fmt.bit_depth, fmt.num_channels,
                       out.ctypes.data)
    return out


class AlacError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"alac_hip status {code}: {msg}")
        self.code = code


class Context:
    """One alac_hip_ctx bound to a device, enqueuing on a torch stream of its own (`self.stream`).

    Stream discipline: the library's kernels run on `self.stream`; every call below first makes that stream wait for the
    caller's current torch stream (inputs produced there — fills, copies — are complete) and afterwards makes the caller's
    stream wait for it (events the caller records on its stream, e.g. bench.py's hand-over to the RCCL side stream, are
    ordered behind the call), and tensors allocated inside a call are allocated and filled on `self.stream`.  Without this
    the library would sit on a private non-blocking stream that nothing the caller does is ordered against."""

    def __init__(self, device=0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("alac_amd needs a HIP device: no GPU visible and there is no CPU fallback")
        self.torch = torch
        self.lib = load_library()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.Stream(device=self.device)
        h = _vp()
        rc = self.lib.alac_hip_create(C.byref(h), device, _vp(self.stream.cuda_stream))
        if rc != 0:
            raise AlacError(rc, "alac_hip_create failed")
        self.h = h
        self._ws = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.alac_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self):
        """context manager around one library call: see the class docstring"""
        import contextlib
        t = self.torch

        @contextlib.contextmanager
        def cm():
            cur = t.cuda.current_stream(self.device)
            if cur == self.stream:  # the caller already works on the context's stream (bench.py's timed loop): nothing to order
                yield cur
                return
            self.stream.wait_stream(cur)
            with t.cuda.stream(self.stream):
                yield cur
            cur.wait_stream(self.stream)
        return cm()

    def _check(self, rc):
        if rc != 0:
            raise AlacError(rc, self.lib.alac_hip_last_error(self.h).decode())

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = self.torch.empty(int(nbytes), dtype=self.torch.uint8, device=self.device)
        return self._ws

    def synchronize(self):
        self._check(self.lib.alac_hip_synchronize(self.h))

    def regime(self, fmt, num_segments):
        """alac_hip_encode_regime: "throughput" / "latency" / "tiny" / "lane" for a batch of independent segments"""
        return self.lib.alac_hip_encode_regime(self.h, C.byref(fmt), int(num_segments)).decode()

    def set_option(self, key, value):
        """alac_hip_set_option: pin a code path of this context (include/alac_hip.h lists the keys)"""
        self._check(self.lib.alac_hip_set_option(self.h, key.encode(), int(value)))

    def get_option(self, key):
        v = _i32(0)
        self._check(self.lib.alac_hip_get_option(self.h, key.encode(), C.byref(v)))
        return v.value

    def options(self, **kw):
        """context manager: set options for the duration of a with-block, then restore them"""
        import contextlib

        @contextlib.contextmanager
        def cm():
            old = {k: self.get_option(k) for k in kw}
            try:
                for k, v in kw.items():
                    self.set_option(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_option(k, v)
        return cm()

    def synth_pcm(self, first_frame, num_frames, fmt, out=None):
        """The synthetic PCM of frames [first_frame, first_frame + num_frames) generated ON THE DEVICE (same bytes as
        synth_pcm(): one generator source) -> uint8 cuda tensor."""
        with self._call() as cur:
            t = self.torch
            if out is None:
                out = t.empty(num_frames * fmt.packet_bytes, dtype=t.uint8, device=self.device)
            assert out.numel() >= num_frames * fmt.packet_bytes
            self._check(self.lib.alac_hip_synth_pcm(self.h, first_frame, num_frames, C.byref(fmt), out.data_ptr()))
            out.record_stream(cur)
            return out

    # ---- encode ----------------------------------------------------------------------------
    def encode_buffers(self, fmt, num_packets):
        """Preallocate outputs so a timed loop does no allocation."""
        t = self.torch
        cap = int(self.lib.alac_hip_encode_max_output_bytes(C.byref(fmt), num_packets))
        return dict(out=t.empty(cap, dtype=t.uint8, device=self.device),
                    sizes=t.empty(num_packets, dtype=t.int32, device=self.device),
                    offsets=t.empty(num_packets + 1, dtype=t.int64, device=self.device))

    def encode(self, fmt, pcm, num_packets, num_samples=None, seg_first=None, state=None, state_in=False,
               bufs=None, max_segment_packets=0):
        """pcm: uint8 cuda tensor (num_packets * fmt.packet_bytes).  Returns the buffers dict
        (out, sizes, offsets); offsets[-1] is the total byte count.  Asynchronous — with a segment table only if
        max_segment_packets (the caller's bound on the longest segment, alac_hip_encode_segmented) is given."""
        with self._call() as cur:
            t = self.torch
            assert pcm.is_cuda and pcm.dtype == t.uint8 and pcm.numel() >= num_packets * fmt.packet_bytes
            nseg = num_packets if seg_first is None else seg_first.numel() - 1
            bufs = bufs or self.encode_buffers(fmt, num_packets)
            # option "lpc": every packet is its own segment, and the workspace is sized for that
            wsb = int(self.lib.alac_hip_encode_workspace_bytes(C.byref(fmt), num_packets,
                                                               num_packets if self.get_option("lpc") else nseg))
            ws = self._workspace(wsb)
            rc = self.lib.alac_hip_encode_segmented(
                self.h, C.byref(fmt), pcm.data_ptr(),
                None if num_samples is None else num_samples.data_ptr(), num_packets,
                None if seg_first is None else seg_first.data_ptr(), nseg, int(max_segment_packets),
                None if state is None else state.data_ptr(), 1 if state_in else 0,
                ws.data_ptr(), ws.numel(), bufs["out"].data_ptr(), bufs["out"].numel(),
                bufs["sizes"].data_ptr(), bufs["offsets"].data_ptr())
            self._check(rc)
            for x in bufs.values():
                if hasattr(x, "record_stream"):
                    x.record_stream(cur)
            return bufs

    def encode_float(self, fmt, x, num_samples=None, seg_first=None, state=None, state_in=False, bufs=None,
                     max_segment_packets=0, clipped=False, dither=None, seed=0, packet_origin=None):
        """encode() from float32 PCM (alac_hip_encode_float): x is a float32 cuda tensor [channels, frames] with any strides
        (x.stride() is passed through: a contiguous [C, T] tensor and the transposed view of a [T, C] one need no copy),
        quantized on the device by the rule of include/alac_hip.h (rint(x * 2^(bit_depth - 1)), saturated, NaN -> 0).
        num_packets = ceil(frames / frame_size); num_samples=None gives the last packet frames mod frame_size frames
        when that is not 0.  Returns encode()'s buffers dict; clipped=True adds "clipped", an int32 [num_packets] tensor of
        the clipped samples per packet.
        dither="tpdf" (alac_hip_encode_float_dither): triangular dither of +-1 LSB in front of the rounding, a pure function
        of (seed, channel, stream frame index) generated on the device; 16, 20 and 24 bits.  packet_origin: an int64 /
        uint64 cuda tensor [num_packets] of every packet's first stream frame index (None: packet p starts at
        p * frame_size), so that a file encoded inside a batch gets the dither it gets alone."""
        if dither not in (None, "none", "tpdf"):
            raise ValueError('encode_float: dither must be None, "none" or "tpdf"')
        with self._call() as cur:
            t = self.torch
            if not (x.is_cuda and x.dtype == t.float32 and x.dim() == 2 and x.shape[0] == fmt.num_channels):
                raise ValueError("encode_float: x must be a float32 cuda tensor [channels, frames]")
            if packet_origin is not None and not (packet_origin.is_cuda and packet_origin.dtype in (t.int64, t.uint64) and
                                                  packet_origin.is_contiguous()):
                raise ValueError("encode_float: packet_origin must be a contiguous int64 / uint64 cuda tensor")
            frames = int(x.shape[1])
            num_packets = (frames + fmt.frame_size - 1) // fmt.frame_size
            if num_samples is None and frames % fmt.frame_size:
                ns = [fmt.frame_size] * (num_packets - 1) + [frames % fmt.frame_size]
                num_samples = t.tensor(ns, dtype=t.int32).to(self.device, non_blocking=True)
            nseg = num_packets if seg_first is None else seg_first.numel() - 1
            bufs = bufs or self.encode_buffers(fmt, num_packets)
            if clipped and "clipped" not in bufs:
                bufs["clipped"] = t.empty(num_packets, dtype=t.int32, device=self.device)
            wsb = int(self.lib.alac_hip_encode_float_workspace_bytes(C.byref(fmt), num_packets,
                                                                     num_packets if self.get_option("lpc") else nseg))
            ws = self._workspace(wsb)
            args = (self.h, C.byref(fmt), x.data_ptr(), int(x.stride(0)), int(x.stride(1)),
                    None if num_samples is None else num_samples.data_ptr(), num_packets,
                    None if seg_first is None else seg_first.data_ptr(), nseg, int(max_segment_packets),
                    None if state is None else state.data_ptr(), 1 if state_in else 0,
                    ws.data_ptr(), ws.numel(), bufs["out"].data_ptr(), bufs["out"].numel(),
                    bufs["sizes"].data_ptr(), bufs["offsets"].data_ptr(), bufs["clipped"].data_ptr() if clipped else None)
            if dither is None:
                rc = self.lib.alac_hip_encode_float(*args)
            else:
                if packet_origin is not None and packet_origin.numel() < num_packets:
                    raise ValueError("encode_float: packet_origin too small")
                dz = Dither(DITHER_TPDF if dither == "tpdf" else DITHER_NONE, 0, int(seed) & 0xFFFFFFFFFFFFFFFF)
                rc = self.lib.alac_hip_encode_float_dither(*args, C.byref(dz),
                                                           None if packet_origin is None else packet_origin.data_ptr())
            self._check(rc)
            for v in bufs.values():
                if hasattr(v, "record_stream"):
                    v.record_stream(cur)
            if num_samples is not None:
                num_samples.record_stream(cur)
            return bufs

    def _int_tensor(self, what, x, channels, container_bytes, channel_stride, frame_stride):
        """the tensor forms of an integer source of `channels` channels -> (container bytes, channel stride, frame stride,
        frames), strides in containers"""
        t = self.torch
        if x.is_cuda and x.dtype in (t.int16, t.int32) and x.dim() == 2 and x.shape[0] == channels:
            cb = 2 if x.dtype == t.int16 else 4
            if container_bytes not in (None, cb) or channel_stride is not None or frame_stride is not None:
                raise ValueError("%s: the container and the strides of an int16 / int32 tensor are the tensor's own" % what)
            frames, cs, fst = int(x.shape[1]), int(x.stride(0)), int(x.stride(1))
        elif x.is_cuda and x.dtype == t.uint8 and x.dim() == 1 and x.is_contiguous() and container_bytes == 3:
            if channel_stride is None or frame_stride is None or frame_stride < 1:
                raise ValueError("%s: packed 3-byte sources need channel_stride= and frame_stride=" % what)
            cb, cs, fst = 3, int(channel_stride), int(frame_stride)
            # the frames the bytes hold: the last channel's row ends inside x
            frames = max(0, (x.numel() // 3 - (channels - 1) * cs - 1) // fst + 1) if x.numel() >= 3 else 0
        else:
            raise ValueError("%s: x must be an int16 / int32 cuda tensor [channels, frames], or a 1-D uint8 cuda tensor "
                             "with container_bytes=3, channel_stride= and frame_stride=" % what)
        return cb, cs, fst, frames

    def _int_source(self, what, fmt, x, bits, left_justified, container_bytes, channel_stride, frame_stride, dither,
                    seed, packet_origin, num_samples):
        """the checks and the alac_hip_int_source that requantize() and encode_int() share ->
        (source struct, frames, num_packets, num_samples, dither struct or None)"""
        t = self.torch
        if dither not in (None, "none", "tpdf"):
            raise ValueError('%s: dither must be None, "none" or "tpdf"' % what)
        if packet_origin is not None and not (packet_origin.is_cuda and packet_origin.dtype in (t.int64, t.uint64) and
                                              packet_origin.is_contiguous()):
            raise ValueError("%s: packet_origin must be a contiguous int64 / uint64 cuda tensor" % what)
        cb, cs, fst, frames = self._int_tensor(what, x, fmt.num_channels, container_bytes, channel_stride, frame_stride)
        num_packets = (frames + fmt.frame_size - 1) // fmt.frame_size
        if num_samples is None and frames % fmt.frame_size:
            ns = [fmt.frame_size] * (num_packets - 1) + [frames % fmt.frame_size]
            num_samples = t.tensor(ns, dtype=t.int32).to(self.device, non_blocking=True)
        if packet_origin is not None and packet_origin.numel() < num_packets:
            raise ValueError("%s: packet_origin too small" % what)
        src = IntSource(cb, 8 * cb if bits is None else int(bits), 1 if left_justified else 0, 0, cs, fst)
        dz = None if dither is None else Dither(DITHER_TPDF if dither == "tpdf" else DITHER_NONE, 0,
                                                int(seed) & 0xFFFFFFFFFFFFFFFF)
        return src, frames, num_packets, num_samples, dz

    def requantize(self, fmt, x, bits=None, left_justified=True, dither=None, seed=0, packet_origin=None, num_samples=None,
                   clipped=False, container_bytes=None, channel_stride=None, frame_stride=None):
        """Integer PCM of any layout, container and depth -> the packed interleaved PCM of fmt that encode() reads and
        verify() expects (alac_hip_pcm_requantize; the rule is in include/alac_hip.h).  x is an int16 or int32 cuda tensor
        [channels, frames] with any strides (x.stride() is passed through), of which `bits` (default: the dtype's width) are
        significant, left-justified (the sample is x >> (width - bits)) or right-justified (values outside the range of
        `bits` saturate and count as clipped); or, for packed little-endian 3-byte containers, a 1-D uint8 cuda tensor with
        container_bytes=3, channel_stride= and frame_stride= in containers.  bits <= fmt.bit_depth widens exactly; a larger
        `bits` is reduced with round half to even, and dither="tpdf" adds the TPDF dither of encode_float (seed,
        packet_origin as there) in front of that rounding.  Returns the uint8 cuda tensor [num_packets * fmt.packet_bytes];
        clipped=True returns (pcm, int32 [num_packets] clipped samples per packet)."""
        with self._call() as cur:
            t = self.torch
            src, _, num_packets, num_samples, dz = self._int_source("requantize", fmt, x, bits, left_justified, container_bytes,
                                                                   channel_stride, frame_stride, dither, seed, packet_origin,
                                                                   num_samples)
            pcm = t.empty(num_packets * fmt.packet_bytes, dtype=t.uint8, device=self.device)
            clip = t.empty(num_packets, dtype=t.int32, device=self.device) if clipped else None
            self._check(self.lib.alac_hip_pcm_requantize(
                self.h, C.byref(fmt), x.data_ptr(), C.byref(src), None if num_samples is None else num_samples.data_ptr(),
                num_packets, pcm.data_ptr(), pcm.numel(), None if clip is None else clip.data_ptr(),
                None if dz is None else C.byref(dz), None if packet_origin is None else packet_origin.data_ptr()))
            for v in (pcm, clip, num_samples):
                if v is not None:
                    v.record_stream(cur)
            return (pcm, clip) if clipped else pcm

    def encode_int(self, fmt, x, bits=None, left_justified=True, num_samples=None, seg_first=None, state=None, state_in=False,
                   bufs=None, max_segment_packets=0, clipped=False, dither=None, seed=0, packet_origin=None,
                   container_bytes=None, channel_stride=None, frame_stride=None):
        """encode() from integer PCM of any layout, container and depth (alac_hip_encode_int): requantize(x) into the tail of
        the workspace, then the encode of it.  x, bits, left_justified, dither, seed, packet_origin and the packed 3-byte
        form as in requantize(); the other arguments and the result as in encode_float()."""
        with self._call() as cur:
            t = self.torch
            src, _, num_packets, num_samples, dz = self._int_source("encode_int", fmt, x, bits, left_justified, container_bytes,
                                                                   channel_stride, frame_stride, dither, seed, packet_origin,
                                                                   num_samples)
            nseg = num_packets if seg_first is None else seg_first.numel() - 1
            bufs = bufs or self.encode_buffers(fmt, num_packets)
            if clipped and "clipped" not in bufs:
                bufs["clipped"] = t.empty(num_packets, dtype=t.int32, device=self.device)
            wsb = int(self.lib.alac_hip_encode_int_workspace_bytes(C.byref(fmt), num_packets,
                                                                   num_packets if self.get_option("lpc") else nseg))
            ws = self._workspace(wsb)
            self._check(self.lib.alac_hip_encode_int(
                self.h, C.byref(fmt), x.data_ptr(), C.byref(src), None if num_samples is None else num_samples.data_ptr(),
                num_packets, None if seg_first is None else seg_first.data_ptr(), nseg, int(max_segment_packets),
                None if state is None else state.data_ptr(), 1 if state_in else 0, ws.data_ptr(), ws.numel(),
                bufs["out"].data_ptr(), bufs["out"].numel(), bufs["sizes"].data_ptr(), bufs["offsets"].data_ptr(),
                bufs["clipped"].data_ptr() if clipped else None, None if dz is None else C.byref(dz),
                None if packet_origin is None else packet_origin.data_ptr()))
            for v in bufs.values():
                if hasattr(v, "record_stream"):
                    v.record_stream(cur)
            if num_samples is not None:
                num_samples.record_stream(cur)
            return bufs

    def probe_float(self, x, seg_first_frame=None):
        """alac_hip_float_probe: what names the lossless bit depth of float32 PCM, per segment of frames.  x is a float32
        cuda tensor [channels, frames] with any strides, passed through like encode_float's; seg_first_frame a sequence of
        num_segments + 1 ascending frame indices (None: one segment, all of x).  Returns an int32 cuda tensor
        [num_segments, 8] viewing the alac_hip_float_report of every segment (words 0-1 over_range, 2-3 nan, 4 need_bits,
        5 peak_bits).  A tensor without frames has only empty segments: reports of zeros.  Asynchronous."""
        with self._call() as cur:
            t = self.torch
            if not (x.is_cuda and x.dtype == t.float32 and x.dim() == 2):
                raise ValueError("probe_float: x must be a float32 cuda tensor [channels, frames]")
            table = None if seg_first_frame is None else np.ascontiguousarray(seg_first_frame, dtype=np.uint64)
            if table is not None and (table.ndim != 1 or table.size < 1):
                raise ValueError("probe_float: seg_first_frame must hold num_segments + 1 frame indices")
            nseg = 1 if table is None else table.size - 1
            reports = t.empty((nseg, 8), dtype=t.int32, device=self.device)
            ws = self._workspace(int(self.lib.alac_hip_float_probe_workspace_bytes(nseg)))
            # a tensor without frames has no address; the call wants one, and reads nothing through it
            base = x if x.shape[1] else t.zeros(4, dtype=t.float32, device=self.device)
            self._check(self.lib.alac_hip_float_probe(
                self.h, base.data_ptr(), int(x.shape[0]), int(x.stride(0)), int(x.stride(1)), int(x.shape[1]),
                None if table is None else table.ctypes.data, nseg, ws.data_ptr(), ws.numel(), reports.data_ptr()))
            reports.record_stream(cur)
            return reports

    def lossless_depth(self, x, seg_first_frame=None):
        """The smallest bit depth of 16, 20, 24, 32 at which encode_float(x) is exactly lossless, per segment
        (alac_hip_float_report_depth over probe_float's reports); 0 where there is none.  Synchronizes."""
        reports = self.probe_float(x, seg_first_frame)
        self.synchronize()
        rows = np.ascontiguousarray(reports.cpu().numpy())
        return [int(self.lib.alac_hip_float_report_depth(rows[s].ctypes.data)) for s in range(rows.shape[0])]

    def probe_int(self, x, bits=None, left_justified=True, seg_first_frame=None, container_bytes=None, channel_stride=None,
                  frame_stride=None, num_channels=None):
        """alac_hip_int_probe: what names the lossless bit depth of integer PCM, per segment of frames.  x, bits,
        left_justified and the packed 3-byte form as in requantize(); the channel count is the tensor's, and for a packed
        3-byte source num_channels= (default: frame_stride where channel_stride is 1, the interleaved form; else 1).
        seg_first_frame as in probe_float().  Returns an int32 cuda tensor [num_segments, 8] viewing the alac_hip_int_report
        of every segment (words 0-1 out_of_range, 2-3 differing_frames, 4 need_bits, 5 peak, 6 pad_bits, 7 zero).  A tensor
        without frames has only empty segments: reports of zeros.  Asynchronous."""
        with self._call() as cur:
            t = self.torch
            if x.dim() == 2:
                channels = int(x.shape[0])
            elif num_channels is not None:
                channels = int(num_channels)
            else:
                channels = int(frame_stride) if channel_stride == 1 and frame_stride else 1
            cb, cs, fst, frames = self._int_tensor("probe_int", x, channels, container_bytes, channel_stride, frame_stride)
            src = IntSource(cb, 8 * cb if bits is None else int(bits), 1 if left_justified else 0, 0, cs, fst)
            table = None if seg_first_frame is None else np.ascontiguousarray(seg_first_frame, dtype=np.uint64)
            if table is not None and (table.ndim != 1 or table.size < 1):
                raise ValueError("probe_int: seg_first_frame must hold num_segments + 1 frame indices")
            nseg = 1 if table is None else table.size - 1
            reports = t.empty((nseg, 8), dtype=t.int32, device=self.device)
            ws = self._workspace(int(self.lib.alac_hip_int_probe_workspace_bytes(nseg)))
            # a tensor without frames has no address; the call wants one, and reads nothing through it
            base = x if x.numel() else t.zeros(4, dtype=t.int32, device=self.device)
            self._check(self.lib.alac_hip_int_probe(
                self.h, base.data_ptr(), C.byref(src), channels, frames, None if table is None else table.ctypes.data, nseg,
                ws.data_ptr(), ws.numel(), reports.data_ptr()))
            reports.record_stream(cur)
            return reports

    def lossless_depth_int(self, x, bits=None, left_justified=True, seg_first_frame=None, container_bytes=None,
                           channel_stride=None, frame_stride=None, num_channels=None):
        """The smallest bit depth of 16, 20, 24, 32 to which requantize(x) / encode_int(x) reduce the source without
        rounding or saturating anything, per segment (alac_hip_int_report_depth over probe_int's reports); 0 where a
        container is out of range or a pad bit is set.  Synchronizes."""
        reports = self.probe_int(x, bits, left_justified, seg_first_frame, container_bytes, channel_stride, frame_stride,
                                 num_channels)
        self.synchronize()
        rows = np.ascontiguousarray(reports.cpu().numpy())
        return [int(self.lib.alac_hip_int_report_depth(rows[s].ctypes.data)) for s in range(rows.shape[0])]

    def _loudness(self, what, channels, sample_rate, frames, seg_first_frame, call):
        """the part loudness_int() and loudness_float() share: the table, the outputs and the workspace; call(table pointer,
        num_segments, workspace, rows tensor, row count, reports tensor) -> status"""
        t = self.torch
        keep, table, nseg, reports = self._measure_table(what, seg_first_frame)
        rows = int(self.lib.alac_hip_loudness_rows(int(sample_rate), frames, table, nseg))
        energy = t.empty((rows, channels), dtype=t.float64, device=self.device)
        ws = self._workspace(max(8, int(self.lib.alac_hip_loudness_workspace_bytes(int(sample_rate), channels, frames, nseg))))
        # a tensor without elements has no address; the call wants one, and writes nothing through it
        target = energy if rows else t.zeros(1, dtype=t.float64, device=self.device)
        self._check(call(table, nseg, ws, target, rows, reports))
        del keep
        return energy, reports

    def _measure_table(self, what, seg_first_frame):
        """what the loudness and the true-peak calls do with seg_first_frame: (the table as a uint64 array or None, its
        address or None, num_segments, the reports tensor [num_segments, 8]).  The caller holds the array over the C call."""
        t = self.torch
        table = None if seg_first_frame is None else np.ascontiguousarray(seg_first_frame, dtype=np.uint64)
        if table is not None and (table.ndim != 1 or table.size < 1):
            raise ValueError("%s: seg_first_frame must hold num_segments + 1 frame indices" % what)
        nseg = 1 if table is None else table.size - 1
        return (table, None if table is None else table.ctypes.data, nseg,
                t.empty((nseg, 8), dtype=t.int32, device=self.device))

    def _true_peak(self, what, channels, seg_first_frame, call):
        """the part true_peak_int() and true_peak_float() share: the table, the outputs and the workspace; call(table pointer,
        num_segments, workspace, channel peaks tensor, reports tensor) -> status"""
        t = self.torch
        keep, table, nseg, reports = self._measure_table(what, seg_first_frame)
        peaks = t.empty((nseg, channels), dtype=t.float64, device=self.device)
        ws = self._workspace(max(8, int(self.lib.alac_hip_true_peak_workspace_bytes(channels, nseg))))
        self._check(call(table, nseg, ws, peaks, reports))
        del keep
        return peaks, reports

    def loudness_int(self, x, sample_rate, bits=None, left_justified=True, seg_first_frame=None, container_bytes=None,
                     channel_stride=None, frame_stride=None, num_channels=None):
        """alac_hip_loudness_int: the K-weighted energy of every 100 ms of every channel (ITU-R BS.1770) and the sample peak
        of integer PCM, per segment of frames.  x, bits, left_justified, the packed 3-byte form and num_channels as in
        probe_int(); seg_first_frame as in probe_float().  Returns (energy, reports): a float64 cuda tensor [rows, channels],
        the rows of all segments back to back, and an int32 cuda tensor [num_segments, 8] viewing the alac_hip_loudness_report
        of every segment (word 0 first_block, 1 num_blocks, 2-3 the peak as a double, 4-5 nonfinite; loudness_reports()
        reads them).  integrated_loudness() gates the rows of one segment.  Asynchronous."""
        with self._call() as cur:
            t = self.torch
            if x.dim() == 2:
                channels = int(x.shape[0])
            elif num_channels is not None:
                channels = int(num_channels)
            else:
                channels = int(frame_stride) if channel_stride == 1 and frame_stride else 1
            cb, cs, fst, frames = self._int_tensor("loudness_int", x, channels, container_bytes, channel_stride, frame_stride)
            src = IntSource(cb, 8 * cb if bits is None else int(bits), 1 if left_justified else 0, 0, cs, fst)
            base = x if x.numel() else t.zeros(4, dtype=t.int32, device=self.device)
            energy, reports = self._loudness(
                "loudness_int", channels, sample_rate, frames, seg_first_frame,
                lambda table, nseg, ws, e, rows, rep: self.lib.alac_hip_loudness_int(
                    self.h, base.data_ptr(), C.byref(src), channels, int(sample_rate), frames, table, nseg, ws.data_ptr(),
                    ws.numel(), e.data_ptr(), rows, rep.data_ptr()))
            energy.record_stream(cur)
            reports.record_stream(cur)
            return energy, reports

    def loudness_float(self, x, sample_rate, seg_first_frame=None):
        """alac_hip_loudness_float: loudness_int() for a float32 cuda tensor [channels, frames] with any strides, passed
        through like probe_float()'s.  Non-finite samples are read as 0.0 and counted in the reports."""
        with self._call() as cur:
            t = self.torch
            if not (x.is_cuda and x.dtype == t.float32 and x.dim() == 2):
                raise ValueError("loudness_float: x must be a float32 cuda tensor [channels, frames]")
            base = x if x.shape[1] else t.zeros(4, dtype=t.float32, device=self.device)
            channels, frames = int(x.shape[0]), int(x.shape[1])
            energy, reports = self._loudness(
                "loudness_float", channels, sample_rate, frames, seg_first_frame,
                lambda table, nseg, ws, e, rows, rep: self.lib.alac_hip_loudness_float(
                    self.h, base.data_ptr(), channels, int(x.stride(0)), int(x.stride(1)), int(sample_rate), frames, table, nseg,
                    ws.data_ptr(), ws.numel(), e.data_ptr(), rows, rep.data_ptr()))
            energy.record_stream(cur)
            reports.record_stream(cur)
            return energy, reports

    @staticmethod
    def loudness_reports(reports):
        """the reports of loudness_int() / loudness_float() on the host: a list of LoudnessReport.  The caller has
        synchronized."""
        raw = np.ascontiguousarray(reports.cpu().numpy())
        return [LoudnessReport.from_buffer_copy(raw[s].tobytes()) for s in range(raw.shape[0])]

    def true_peak_int(self, x, sample_rate, bits=None, left_justified=True, seg_first_frame=None, container_bytes=None,
                      channel_stride=None, frame_stride=None, num_channels=None):
        """alac_hip_true_peak_int: the true peak (ITU-R BS.1770-4 annex 2) of integer PCM, per segment of frames and
        channel.  The arguments of loudness_int().  Returns (channel_peak, reports): a float64 cuda tensor [num_segments,
        channels] and an int32 cuda tensor [num_segments, 8] viewing the alac_hip_true_peak_report of every segment (words 0-1
        the true peak as a double, 2-3 the sample peak, 4-5 nonfinite; true_peak_reports() reads them).  Asynchronous."""
        with self._call() as cur:
            t = self.torch
            if x.dim() == 2:
                channels = int(x.shape[0])
            elif num_channels is not None:
                channels = int(num_channels)
            else:
                channels = int(frame_stride) if channel_stride == 1 and frame_stride else 1
            cb, cs, fst, frames = self._int_tensor("true_peak_int", x, channels, container_bytes, channel_stride, frame_stride)
            src = IntSource(cb, 8 * cb if bits is None else int(bits), 1 if left_justified else 0, 0, cs, fst)
            base = x if x.numel() else t.zeros(4, dtype=t.int32, device=self.device)
            peaks, reports = self._true_peak(
                "true_peak_int", channels, seg_first_frame,
                lambda table, nseg, ws, pk, rep: self.lib.alac_hip_true_peak_int(
                    self.h, base.data_ptr(), C.byref(src), channels, int(sample_rate), frames, table, nseg, ws.data_ptr(),
                    ws.numel(), pk.data_ptr(), rep.data_ptr()))
            peaks.record_stream(cur)
            reports.record_stream(cur)
            return peaks, reports

    def true_peak_float(self, x, sample_rate, seg_first_frame=None):
        """alac_hip_true_peak_float: true_peak_int() for a float32 cuda tensor [channels, frames] with any strides, passed
        through like probe_float()'s.  Non-finite samples are read as 0.0 and counted in the reports."""
        with self._call() as cur:
            t = self.torch
            if not (x.is_cuda and x.dtype == t.float32 and x.dim() == 2):
                raise ValueError("true_peak_float: x must be a float32 cuda tensor [channels, frames]")
            base = x if x.shape[1] else t.zeros(4, dtype=t.float32, device=self.device)
            channels, frames = int(x.shape[0]), int(x.shape[1])
            peaks, reports = self._true_peak(
                "true_peak_float", channels, seg_first_frame,
                lambda table, nseg, ws, pk, rep: self.lib.alac_hip_true_peak_float(
                    self.h, base.data_ptr(), channels, int(x.stride(0)), int(x.stride(1)), int(sample_rate), frames, table, nseg,
                    ws.data_ptr(), ws.numel(), pk.data_ptr(), rep.data_ptr()))
            peaks.record_stream(cur)
            reports.record_stream(cur)
            return peaks, reports

    @staticmethod
    def true_peak_reports(reports):
        """the reports of true_peak_int() / true_peak_float() on the host: a list of TruePeakReport.  The caller has
        synchronized."""
        raw = np.ascontiguousarray(reports.cpu().numpy())
        return [TruePeakReport.from_buffer_copy(raw[s].tobytes()) for s in range(raw.shape[0])]

    def _resample(self, what, channels, in_rate, out_rate, frames, seg_first_frame, call):
        """the part resample_int() and resample_float() share: the table, the outputs and the workspace; call(table pointer,
        num_segments, workspace, output tensor, its frames, reports tensor) -> status"""
        t = self.torch
        keep, table, nseg, reports = self._measure_table(what, seg_first_frame)
        total = int(self.lib.alac_hip_resample_frames(int(in_rate), int(out_rate), frames, table, nseg, None))
        y = t.empty((channels, total), dtype=t.float32, device=self.device)
        ws = self._workspace(max(16, int(self.lib.alac_hip_resample_workspace_bytes(int(in_rate), int(out_rate), channels, nseg))))
        # a tensor without elements has no address; the call wants one, and writes nothing through it
        target = y if total else t.zeros(1, dtype=t.float32, device=self.device)
        self._check(call(table, nseg, ws, target, total, reports))
        del keep
        return y, reports

    def resample_int(self, x, in_rate, out_rate, bits=None, left_justified=True, seg_first_frame=None, container_bytes=None,
                     channel_stride=None, frame_stride=None, num_channels=None):
        """alac_hip_resample_int: integer PCM at in_rate -> float32 planar PCM at out_rate, per segment of frames, by the
        windowed-sinc rule of include/alac_hip.h.  The arguments of true_peak_int().  Returns (y, reports): a float32 cuda
        tensor [channels, out_total], the segments back to back at the offsets of resample_frames(), which is what
        encode_float() takes, and an int32 cuda tensor [num_segments, 8] viewing the alac_hip_resample_report of every segment
        (resample_reports() reads them).  Asynchronous."""
        with self._call() as cur:
            t = self.torch
            if x.dim() == 2:
                channels = int(x.shape[0])
            elif num_channels is not None:
                channels = int(num_channels)
            else:
                channels = int(frame_stride) if channel_stride == 1 and frame_stride else 1
            cb, cs, fst, frames = self._int_tensor("resample_int", x, channels, container_bytes, channel_stride, frame_stride)
            src = IntSource(cb, 8 * cb if bits is None else int(bits), 1 if left_justified else 0, 0, cs, fst)
            base = x if x.numel() else t.zeros(4, dtype=t.int32, device=self.device)
            y, reports = self._resample(
                "resample_int", channels, in_rate, out_rate, frames, seg_first_frame,
                lambda table, nseg, ws, out, total, rep: self.lib.alac_hip_resample_int(
                    self.h, base.data_ptr(), C.byref(src), channels, int(in_rate), int(out_rate), frames, table, nseg,
                    ws.data_ptr(), ws.numel(), out.data_ptr(), total, total, rep.data_ptr()))
            y.record_stream(cur)
            reports.record_stream(cur)
            return y, reports

    def resample_float(self, x, in_rate, out_rate, seg_first_frame=None):
        """alac_hip_resample_float: resample_int() for a float32 cuda tensor [channels, frames] with any strides, passed
        through like probe_float()'s.  Non-finite samples are read as 0.0 and counted in the reports."""
        with self._call() as cur:
            t = self.torch
            if not (x.is_cuda and x.dtype == t.float32 and x.dim() == 2):
                raise ValueError("resample_float: x must be a float32 cuda tensor [channels, frames]")
            base = x if x.shape[1] else t.zeros(4, dtype=t.float32, device=self.device)
            channels, frames = int(x.shape[0]), int(x.shape[1])
            y, reports = self._resample(
                "resample_float", channels, in_rate, out_rate, frames, seg_first_frame,
                lambda table, nseg, ws, out, total, rep: self.lib.alac_hip_resample_float(
                    self.h, base.data_ptr(), channels, int(x.stride(0)), int(x.stride(1)), int(in_rate), int(out_rate), frames,
                    table, nseg, ws.data_ptr(), ws.numel(), out.data_ptr(), total, total, rep.data_ptr()))
            y.record_stream(cur)
            reports.record_stream(cur)
            return y, reports

    @staticmethod
    def resample_reports(reports):
        """the reports of resample_int() / resample_float() on the host: a list of ResampleReport.  The caller has
        synchronized."""
        raw = np.ascontiguousarray(reports.cpu().numpy())
        return [ResampleReport.from_buffer_copy(raw[s].tobytes()) for s in range(raw.shape[0])]

    def pcm_crc32_device(self, pcm, ranges=None):
        """alac_hip_pcm_crc32: zlib.crc32 of ranges of a uint8 cuda tensor, computed where it lies.  ranges: a sequence of
        (offset, length) in bytes, ascending and non-overlapping (gaps and empty ranges allowed); None: all of pcm.
        Returns an int32 cuda tensor [num_ranges, 4] viewing the alac_hip_pcm_digest of every range (words 0-1 bytes,
        2 crc32, 3 zero).  Asynchronous."""
        with self._call() as cur:
            t = self.torch
            if not (pcm.is_cuda and pcm.dtype == t.uint8 and pcm.dim() == 1 and pcm.is_contiguous()):
                raise ValueError("pcm_crc32: pcm must be a contiguous one-dimensional uint8 cuda tensor")
            table = None if ranges is None else np.ascontiguousarray(ranges, dtype=np.uint64).reshape(-1, 2)
            if table is not None and table.shape[0] < 1:
                raise ValueError("pcm_crc32: ranges must hold at least one (offset, length)")
            n = 1 if table is None else table.shape[0]
            digests = t.empty((n, 4), dtype=t.int32, device=self.device)
            ws = self._workspace(int(self.lib.alac_hip_pcm_crc32_workspace_bytes(n)))
            self._check(self.lib.alac_hip_pcm_crc32(
                self.h, pcm.data_ptr() if pcm.numel() else None, int(pcm.numel()),
                None if table is None else table.ctypes.data, n, ws.data_ptr(), ws.numel(), digests.data_ptr()))
            digests.record_stream(cur)
            return digests

    def pcm_crc32(self, pcm, ranges=None):
        """pcm_crc32_device's digests on the host: a list of (crc32, bytes), one per range.  Synchronizes; only the digests
        cross the bus."""
        digests = self.pcm_crc32_device(pcm, ranges)
        self.synchronize()
        rows = digests.cpu().numpy().view(np.uint32)
        return [(int(r[2]), int(r[0]) | (int(r[1]) << 32)) for r in rows]

    def encode_to_host(self, fmt, pcm, num_packets, **kw):
        """Convenience for tests: returns (stream bytes ndarray, sizes ndarray)."""
        b = self.encode(fmt, pcm, num_packets, **kw)
        self.synchronize()
        total = int(b["offsets"][-1].item())
        return b["out"][:total].cpu().numpy(), b["sizes"].cpu().numpy().astype(np.uint32)

    def encode_host(self, fmt, pcm, total_samples, segment_packets=0, state=None):
        """alac_hip_encode_host: host PCM (uint8 ndarray, total_samples sample-frames) -> (stream ndarray, sizes ndarray,
        final state ndarray).  segment_packets = 0: ONE chained segment (a whole file); k: state reset every k packets.
        Synchronous (does its own H2D / D2H)."""
        pcm = np.ascontiguousarray(pcm, np.uint8)
        npk = (total_samples + fmt.frame_size - 1) // fmt.frame_size
        nseg = (npk + segment_packets - 1) // segment_packets if segment_packets else 1
        cap = int(self.lib.alac_hip_encode_max_output_bytes(C.byref(fmt), npk))
        out = np.zeros(cap, np.uint8)
        sizes = np.zeros(max(npk, 1), np.uint32)
        n16 = int(self.lib.alac_hip_state_int16(C.byref(fmt)))
        st = np.zeros(nseg * n16, np.int16) if state is None else np.ascontiguousarray(state, np.int16).copy()
        total = _u64(0)
        self._check(self.lib.alac_hip_encode_host(self.h, C.byref(fmt), pcm.ctypes.data, total_samples, segment_packets,
                                                  st.ctypes.data, 0 if state is None else 1, out.ctypes.data, cap,
                                                  sizes.ctypes.data, C.byref(total)))
        return out[:total.value].copy(), sizes[:npk].copy(), st

    def profile_begin(self, max_calls):
        self._check(self.lib.alac_hip_profile_begin(self.h, max_calls))

    def profile_end(self):
        """-> (calls, {stage name: (mean ms per launch, launches per call)}); synchronises."""
        n = _u32(0)
        ns = self.lib.alac_hip_num_stages()
        ms = (C.c_float * ns)()
        ln = (_u32 * ns)()
        self._check(self.lib.alac_hip_profile_end(self.h, C.byref(n), ms, ln))
        return n.value, {self.lib.alac_hip_stage_name(i).decode(): (float(ms[i]), int(ln[i])) for i in range(ns)}

    def magic_cookie(self, fmt, max_frame_bytes=0, avg_bit_rate=0):
        c = np.zeros(48, np.uint8)
        n = self.lib.alac_hip_magic_cookie_full(C.byref(fmt), max_frame_bytes, avg_bit_rate, c.ctypes.data, 48)
        assert n == self.lib.alac_hip_magic_cookie_size(C.byref(fmt)) and n in (24, 48)
        return c[:n].copy()

    # ---- decode ----------------------------------------------------------------------------
    def decode(self, cookie, stream, offsets, num_packets, zero_fill=True, out=None):
        """stream: uint8 cuda tensor, offsets: int64 cuda tensor [num_packets+1].
        Returns (pcm uint8 tensor [num_packets*packet_bytes], num_samples int32, status int32).
        zero_fill=False leaves the bytes behind a short packet's samples uninitialised (the library writes
        num_samples frames per packet and zeroes only failed packets) and saves a pass over the output.
        out=(pcm, num_samples, status): write into these tensors instead of allocating (a timed loop that allocates
        2 GB per call measures the allocator)."""
        with self._call() as cur:
            t = self.torch
            ck = np.ascontiguousarray(cookie, np.uint8)
            fmt = Format()
            self._check(self.lib.alac_hip_format_from_cookie(ck.ctypes.data, ck.size, C.byref(fmt)))
            if out is not None:
                pcm, ns, st = out
                if pcm.numel() < num_packets * fmt.packet_bytes or ns.numel() < num_packets or st.numel() < num_packets:
                    raise ValueError("decode: output tensors too small")
            else:
                alloc = t.zeros if zero_fill else t.empty
                pcm = alloc(num_packets * fmt.packet_bytes, dtype=t.uint8, device=self.device)
                ns = t.zeros(num_packets, dtype=t.int32, device=self.device)
                st = t.zeros(num_packets, dtype=t.int32, device=self.device)
            # sized from the stream actually handed over (ID_FIL / ID_DSE padding may exceed the regular bound)
            wsb = int(self.lib.alac_hip_decode_workspace_bytes_stream(C.byref(fmt), num_packets, int(stream.numel())))
            ws = self._workspace(wsb)
            rc = self.lib.alac_hip_decode(self.h, ck.ctypes.data, ck.size, stream.data_ptr(), offsets.data_ptr(),
                                          num_packets, ws.data_ptr(), ws.numel(), pcm.data_ptr(), ns.data_ptr(),
                                          st.data_ptr())
            self._check(rc)
            for x in (pcm, ns, st):
                x.record_stream(cur)  # allocated on self.stream, consumed on the caller's
            return pcm, ns, st, fmt

    def decode_float(self, cookie, stream, offsets, num_packets, zero_fill=True, out=None, channel_stride=None):
        """decode() straight to planar float32 (alac_hip_decode_float): sample / 2^(bit_depth - 1), what torchaudio.load
        returns.  Returns (pcm float32 tensor [channels, num_packets * frame_size], num_samples int32, status int32, fmt).
        channel_stride: floats between two channels' rows (default num_packets * frame_size); with a larger one pcm is a
        view of the [channels, channel_stride] buffer.  zero_fill=False leaves the samples behind a short packet's frames
        uninitialised.  out=(buffer, num_samples, status): write into these tensors instead of allocating; buffer is a
        float32 cuda tensor of at least (channels - 1) * channel_stride + num_packets * frame_size elements."""
        with self._call() as cur:
            t = self.torch
            ck = np.ascontiguousarray(cookie, np.uint8)
            fmt = Format()
            self._check(self.lib.alac_hip_format_from_cookie(ck.ctypes.data, ck.size, C.byref(fmt)))
            frames = num_packets * fmt.frame_size
            stride = frames if channel_stride is None else int(channel_stride)
            need = (fmt.num_channels - 1) * stride + frames
            if out is not None:
                buf, ns, st = out
                if buf.dtype != t.float32 or not buf.is_contiguous():
                    raise ValueError("decode_float: out buffer must be a contiguous float32 tensor")
                if buf.numel() < need or ns.numel() < num_packets or st.numel() < num_packets:
                    raise ValueError("decode_float: output tensors too small")
            else:
                alloc = t.zeros if zero_fill else t.empty
                buf = alloc(max(fmt.num_channels * stride, need), dtype=t.float32, device=self.device)
                ns = t.zeros(num_packets, dtype=t.int32, device=self.device)
                st = t.zeros(num_packets, dtype=t.int32, device=self.device)
            wsb = int(self.lib.alac_hip_decode_workspace_bytes_stream(C.byref(fmt), num_packets, int(stream.numel())))
            ws = self._workspace(wsb)
            rc = self.lib.alac_hip_decode_float(self.h, ck.ctypes.data, ck.size, stream.data_ptr(), offsets.data_ptr(),
                                                num_packets, ws.data_ptr(), ws.numel(), buf.data_ptr(), stride,
                                                ns.data_ptr(), st.data_ptr())
            self._check(rc)
            for x in (buf, ns, st):
                x.record_stream(cur)
            pcm = buf.as_strided((fmt.num_channels, frames), (stride, 1))
            return pcm, ns, st, fmt

    def decode_int(self, cookie, stream, offsets, num_packets, dtype=None, layout="planar", bits=None, left_justified=True,
                   zero_fill=True, out=None, channel_stride=None):
        """decode() straight to integer PCM of the caller's layout (alac_hip_decode_int; the rule is in include/alac_hip.h):
        what torchaudio.load(normalize=False) or soundfile.read(dtype="int32") return, or the containers of a 24-in-32
        file.  dtype torch.int32 (the default) or torch.int16: a [channels, frames] tensor for layout="planar" (rows
        channel_stride containers apart, default frames) or [frames, channels] for "interleaved"; dtype torch.uint8: packed
        little-endian 3-byte containers, [frames, channels, 3] ([channels, frames, 3] for "planar").  The decoded sample
        goes left-justified into its container (sample << (container bits - depth)) or, with left_justified=False,
        right-justified at `bits` significant bits (sample << (bits - depth)), sign-extended.
        bits defaults to the container's width when left_justified (32 / 16 / 24), else to the stream's depth.
        zero_fill=False leaves the containers behind a short packet's frames uninitialised.  out=(tensor, num_samples,
        status): write into these instead of allocating; tensor has the shape above and any strides in which no two
        samples share a container (a view into a larger batch tensor works).
        Returns (tensor, num_samples int32, status int32, fmt).  Asynchronous like decode()."""
        with self._call() as cur:
            t = self.torch
            ck = np.ascontiguousarray(cookie, np.uint8)
            fmt = Format()
            self._check(self.lib.alac_hip_format_from_cookie(ck.ctypes.data, ck.size, C.byref(fmt)))
            dtype = t.int32 if dtype is None else dtype
            if dtype not in (t.int32, t.int16, t.uint8):
                raise ValueError("decode_int: dtype must be torch.int32, torch.int16 or torch.uint8 (packed 3-byte containers)")
            if layout not in ("planar", "interleaved"):
                raise ValueError('decode_int: layout must be "planar" or "interleaved"')
            cb = {t.int32: 4, t.int16: 2, t.uint8: 3}[dtype]
            unit = 3 if cb == 3 else 1  # elements of the tensor per container
            ch, frames = fmt.num_channels, num_packets * fmt.frame_size
            planar = layout == "planar"
            shape = ((ch, frames) if planar else (frames, ch)) + ((3,) if cb == 3 else ())
            if out is not None:
                pcm, ns, st = out
                if channel_stride is not None:
                    raise ValueError("decode_int: the strides of out= are the tensor's own")
                if not pcm.is_cuda or pcm.dtype != dtype or tuple(pcm.shape) != shape:
                    raise ValueError("decode_int: out tensor must be a cuda tensor of dtype %s and shape %s" % (dtype, shape))
                if cb == 3 and (pcm.stride(2) != 1 or pcm.stride(0) % 3 or pcm.stride(1) % 3):
                    raise ValueError("decode_int: packed 3-byte containers lie multiples of 3 bytes apart, their bytes together")
                if ns.numel() < num_packets or st.numel() < num_packets:
                    raise ValueError("decode_int: output tensors too small")
                s0, s1 = pcm.stride(0) // unit, pcm.stride(1) // unit
                cs, fst = (s0, s1) if planar else (s1, s0)
            else:
                alloc = t.zeros if zero_fill else t.empty
                if planar:
                    cs, fst = (frames if channel_stride is None else int(channel_stride)), 1
                    if cs < frames:
                        raise ValueError("decode_int: channel_stride below num_packets * frame_size")
                    buf = alloc(ch * cs * unit, dtype=dtype, device=self.device)
                    pcm = buf.as_strided(shape, (cs * unit, unit) + ((1,) if cb == 3 else ()))
                else:
                    if channel_stride is not None:
                        raise ValueError("decode_int: channel_stride= belongs to the planar layout")
                    cs, fst = 1, ch
                    pcm = alloc(shape, dtype=dtype, device=self.device)
                ns = t.zeros(num_packets, dtype=t.int32, device=self.device)
                st = t.zeros(num_packets, dtype=t.int32, device=self.device)
            S = (8 * cb if left_justified else fmt.bit_depth) if bits is None else int(bits)
            dst = IntSource(cb, S, 1 if left_justified else 0, 0, cs, fst)
            wsb = int(self.lib.alac_hip_decode_workspace_bytes_stream(C.byref(fmt), num_packets, int(stream.numel())))
            ws = self._workspace(wsb)
            rc = self.lib.alac_hip_decode_int(self.h, ck.ctypes.data, ck.size, stream.data_ptr(), offsets.data_ptr(),
                                              num_packets, ws.data_ptr(), ws.numel(), pcm.data_ptr(), C.byref(dst),
                                              ns.data_ptr(), st.data_ptr())
            self._check(rc)
            for x in (pcm, ns, st):
                x.record_stream(cur)
            return pcm, ns, st, fmt

    def verify(self, cookie, stream, offsets, num_packets, pcm, num_samples=None):
        """Decode on the device and compare with `pcm` (uint8 cuda, the layout decode() returns), writing no PCM.
        num_samples: expected frames per packet (int32 cuda [num_packets]), None = every packet full.
        Returns (first_mismatch, status, bad_packets): int32 cuda tensors [num_packets], [num_packets], [1];
        first_mismatch[p] is the lowest differing sample-frame, -1 (0xFFFFFFFF) where the packet matches, 0 where it did not
        decode; bad_packets counts the packets that are not -1.  Asynchronous like decode()."""
        with self._call() as cur:
            t = self.torch
            ck = np.ascontiguousarray(cookie, np.uint8)
            fmt = Format()
            self._check(self.lib.alac_hip_format_from_cookie(ck.ctypes.data, ck.size, C.byref(fmt)))
            if pcm.numel() < num_packets * fmt.packet_bytes:
                raise ValueError("verify: expected PCM too small")
            if num_samples is not None and num_samples.numel() < num_packets:
                raise ValueError("verify: num_samples too small")
            # every word is written by the call (no fill launches in front of it)
            fm = t.empty(num_packets, dtype=t.int32, device=self.device)
            st = t.empty(num_packets, dtype=t.int32, device=self.device)
            bad = t.empty(1, dtype=t.int32, device=self.device)
            wsb = int(self.lib.alac_hip_verify_workspace_bytes_stream(C.byref(fmt), num_packets, int(stream.numel())))
            ws = self._workspace(wsb)
            rc = self.lib.alac_hip_verify(self.h, ck.ctypes.data, ck.size, stream.data_ptr(), offsets.data_ptr(), num_packets,
                                          pcm.data_ptr(), None if num_samples is None else num_samples.data_ptr(),
                                          ws.data_ptr(), ws.numel(), fm.data_ptr(), st.data_ptr(), bad.data_ptr())
            self._check(rc)
            for x in (fm, st, bad):
                x.record_stream(cur)
            return fm, st, bad

    def verify_float(self, cookie, stream, offsets, num_packets, x, num_samples=None, dither=None, seed=0,
                     packet_origin=None):
        """verify() against the float32 source of encode_float (alac_hip_verify_float): x is a float32 cuda tensor
        [channels, frames] of any strides, passed through like encode_float's.  Every decoded sample is compared with what
        the float encode path stages for its source float at the stream's bit depth — rounding, saturation, NaN -> 0 and,
        with dither="tpdf", the dither of (seed, channel, stream frame index); packet_origin as in encode_float.
        num_samples: expected frames per packet (int32 cuda [num_packets]); None = every packet full, the last one
        frames mod frame_size where x ends inside it.  Only frames in front of a packet's expected count are read from
        x, so with num_samples given x must hold those.  Returns verify()'s triple.  Asynchronous like decode()."""
        if dither not in (None, "none", "tpdf"):
            raise ValueError('verify_float: dither must be None, "none" or "tpdf"')
        with self._call() as cur:
            t = self.torch
            ck = np.ascontiguousarray(cookie, np.uint8)
            fmt = Format()
            self._check(self.lib.alac_hip_format_from_cookie(ck.ctypes.data, ck.size, C.byref(fmt)))
            if not (x.is_cuda and x.dtype == t.float32 and x.dim() == 2 and x.shape[0] == fmt.num_channels):
                raise ValueError("verify_float: x must be a float32 cuda tensor [channels, frames]")
            if packet_origin is not None and not (packet_origin.is_cuda and packet_origin.dtype in (t.int64, t.uint64) and
                                                  packet_origin.is_contiguous() and packet_origin.numel() >= num_packets):
                raise ValueError("verify_float: packet_origin must be a contiguous int64 / uint64 cuda tensor [num_packets]")
            frames = int(x.shape[1])
            if num_samples is None and frames < num_packets * fmt.frame_size:
                full = frames // fmt.frame_size
                ns = [fmt.frame_size] * full + [frames % fmt.frame_size] + [0] * (num_packets - full - 1)
                num_samples = t.tensor(ns[:num_packets], dtype=t.int32).to(self.device, non_blocking=True)
            if num_samples is not None and num_samples.numel() < num_packets:
                raise ValueError("verify_float: num_samples too small")
            fm = t.empty(num_packets, dtype=t.int32, device=self.device)
            st = t.empty(num_packets, dtype=t.int32, device=self.device)
            bad = t.empty(1, dtype=t.int32, device=self.device)
            wsb = int(self.lib.alac_hip_verify_workspace_bytes_stream(C.byref(fmt), num_packets, int(stream.numel())))
            ws = self._workspace(wsb)
            dz = None
            if dither is not None:
                dz = Dither(DITHER_TPDF if dither == "tpdf" else DITHER_NONE, 0, int(seed) & 0xFFFFFFFFFFFFFFFF)
            rc = self.lib.alac_hip_verify_float(self.h, ck.ctypes.data, ck.size, stream.data_ptr(), offsets.data_ptr(),
                                                num_packets, x.data_ptr(), int(x.stride(0)), int(x.stride(1)),
                                                None if num_samples is None else num_samples.data_ptr(),
                                                None if dz is None else C.byref(dz),
                                                None if packet_origin is None else packet_origin.data_ptr(),
                                                ws.data_ptr(), ws.numel(), fm.data_ptr(), st.data_ptr(), bad.data_ptr())
            self._check(rc)
            for v in (fm, st, bad):
                v.record_stream(cur)
            if num_samples is not None:
                num_samples.record_stream(cur)
            return fm, st, bad

    # ---- stage level ------------------------------------------------------------------------
    def pc_block(self, x, num, coefs, numactive, chanbits, denshift=9, decode=False):
        """x: int32 cuda [rows, stride]; coefs: int16 cuda [rows, 32] (adapted in place)."""
        with self._call() as cur:
            t = self.torch
            out = t.zeros_like(x)
            fn = self.lib.alac_hip_unpc_block if decode else self.lib.alac_hip_pc_block
            self._check(fn(self.h, x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], num,
                           coefs.data_ptr(), numactive, chanbits, denshift))
            out.record_stream(cur)
            return out

    def dyn_comp(self, pc, num_samples, bit_size, bytes_stride, mb0=10, pb=40, kb=14):
        with self._call() as cur:
            t = self.torch
            rows = pc.shape[0]
            bits = t.zeros((rows, bytes_stride), dtype=t.uint8, device=self.device)
            nb = t.zeros(rows, dtype=t.int32, device=self.device)
            self._check(self.lib.alac_hip_dyn_comp(self.h, mb0, pb, kb, pc.data_ptr(), rows, pc.shape[1],
                                                   num_samples, bit_size, bits.data_ptr(), bytes_stride,
                                                   nb.data_ptr()))
            bits.record_stream(cur)
            nb.record_stream(cur)
            return bits, nb

    def dyn_decomp(self, bits, num_samples, max_size, mb0=10, pb=40, kb=14):
        with self._call() as cur:
            t = self.torch
            rows, stride = bits.shape
            pc = t.zeros((rows, max(num_samples, 1)), dtype=t.int32, device=self.device)
            nb = t.zeros(rows, dtype=t.int32, device=self.device)
            st = t.zeros(rows, dtype=t.int32, device=self.device)
            self._check(self.lib.alac_hip_dyn_decomp(self.h, mb0, pb, kb, bits.data_ptr(), stride, rows,
                                                     pc.data_ptr(), pc.shape[1], num_samples, max_size,
                                                     nb.data_ptr(), st.data_ptr()))
            for x in (pc, nb, st):
                x.record_stream(cur)  # allocated on self.stream, consumed on the caller's
            return pc, nb, st


class Comm:
    """One alac_hip_comm (RCCL communicator of the re-assembly, include/alac_hip.h): one per process / GPU.

    `unique_id()` on rank 0 -> bytes every rank passes to the constructor (distributed by the caller's launcher channel).
    begin() / finish() enqueue on the torch stream that is current when they are called and never touch torch.distributed."""

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        rc = load_library().alac_hip_comm_unique_id(buf)
        if rc != 0:
            raise AlacError(rc, "alac_hip_comm_unique_id (librccl missing?)")
        return bytes(buf)

    def __init__(self, device, unique_id, rank, world):
        import torch
        self.torch = torch
        self.lib = load_library()
        self.device = torch.device("cuda", device)
        h = _vp()
        idb = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        rc = self.lib.alac_hip_comm_create(C.byref(h), device, idb, rank, world)
        if rc != 0:
            raise AlacError(rc, "alac_hip_comm_create failed")
        self.h, self.rank, self.world = h, rank, world

    def close(self):
        if getattr(self, "h", None):
            self.lib.alac_hip_comm_destroy(self.h)
            self.h = None

    def _check(self, rc):
        if rc != 0:
            raise AlacError(rc, self.lib.alac_hip_comm_last_error(self.h).decode())

    def _stream(self):
        return _vp(self.torch.cuda.current_stream(self.device).cuda_stream)

    def begin(self, slot, offsets, num_packets, shard_capacity, out_capacity, sizes=None, all_sizes=None):
        """offsets: the int64 [num_packets + 1] tensor alac_hip_encode wrote (its last entry is the shard's byte count)"""
        self._check(self.lib.alac_hip_reassemble_begin(
            self.h, slot, offsets.data_ptr() + 8 * num_packets, int(shard_capacity), int(out_capacity),
            None if sizes is None else sizes.data_ptr(), num_packets, None if all_sizes is None else all_sizes.data_ptr(),
            self._stream()))

    def finish(self, slot, shard, stream_out):
        """-> byte offsets of the shards in stream_out, [world + 1]"""
        offs = (_u64 * (self.world + 1))()
        self._check(self.lib.alac_hip_reassemble_finish(self.h, slot, shard.data_ptr(), stream_out.data_ptr(), offs, self._stream()))
        return list(offs)
