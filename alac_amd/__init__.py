"""alac_amd — MI355X-native ALAC encode/decode hot path.

The product is libalac_hip.so (HIP kernels for gfx950 behind the C-ABI of include/alac_hip.h,
plus the C++ ALACEncoder/ALACDecoder classes).  This package is the thin Python binding used by
the tests and bench.py; it never falls back to a CPU implementation.
"""
from .capi import (AlacError, Comm, Context, Dither, FloatReport, Format, IntReport, IntSource, LIB_PATH, LoudnessReport,  # noqa: F401
                   PcmDigest, ResampleReport, SIGNATURES, TruePeakReport, crc32_combine, integrated_loudness,
                   load_library, loudness_filter, loudness_rows, make_format, resample_filter, resample_frames, shard_offsets,
                   shard_range, source_fingerprint, synth_pcm, true_peak_filter)

__all__ = ["AlacError", "Comm", "Context", "Dither", "FloatReport", "Format", "IntReport", "IntSource", "LIB_PATH", "LoudnessReport",
           "PcmDigest", "ResampleReport", "SIGNATURES", "TruePeakReport", "crc32_combine", "integrated_loudness",
           "load_library", "loudness_filter", "loudness_rows", "make_format", "resample_filter", "resample_frames",
           "shard_offsets", "shard_range", "source_fingerprint", "synth_pcm", "true_peak_filter"]
