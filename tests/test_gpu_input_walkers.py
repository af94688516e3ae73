"""GPU: the general layout of the two conversion passes (pcm_walk, alac_pcm_walk.hpp) where a packet ends inside a lane's
group of 4 frames and in its second block.  A frame size of 1030 is no multiple of 4, so every source takes the general
layout, channel by channel; a packet is two blocks, the second of 6 frames (one whole group and one of which 2 frames lie in
the packet).  Both sources are [3, T], 3 packets, the last of 5 frames.  Float: the bytes equal encode() of the numpy-quantized
PCM and the clip counts equal numpy's (the helpers of test_gpu_encode_float.py at this frame size).  Integer: packed 3-byte
containers, frames contiguous, reduced to 16 bits with and without dither, against tests/pcm_requant_ref.py (the check of
test_gpu_encode_int.py)."""
import numpy as np
import pytest
import torch

import alac_amd
import test_gpu_encode_float as F
import test_gpu_encode_int as I

pytestmark = pytest.mark.gpu
FS = 1030
COUNTS = [FS, FS, 5]


@pytest.mark.parametrize("depth", [16, 32])
def test_float_general_layout_two_blocks(gpu_ctx, depth, monkeypatch):
    monkeypatch.setattr(F, "FS", FS)  # pack() and reference() of that module at this frame size
    fmt = alac_amd.make_format(FS, depth, 3, 44100)
    frames = 2 * FS + COUNTS[2]
    x = F.make_x(depth, 3, frames, 40 + depth)
    b = gpu_ctx.encode_float(fmt, torch.from_numpy(x).cuda(), clipped=True)
    F.assert_same(F.fetch(gpu_ctx, b), F.reference(gpu_ctx, fmt, x), depth)
    _, clip = F.quantize(x, depth)
    want = [int(clip[:, p * FS:p * FS + k].sum()) for p, k in enumerate(COUNTS)]
    assert b["clipped"].cpu().tolist() == want
    assert sum(want) > 0


@pytest.mark.parametrize("dither", [False, True])
def test_integer_general_layout_two_blocks(gpu_ctx, dither):
    assert I.NP == len(COUNTS)
    for lj in (True, False):
        clips = I.check(gpu_ctx, 3, 24, lj, 16, 3, FS, COUNTS, "interleaved", dither, [0, FS + 1, 5 * FS] if dither else None,
                        77 + lj)
        assert np.asarray(clips)[:2].min() > 0  # the top tie clips in every whole packet
