"""Stage timing (alac_hip_profile_begin / _end): the launchers record an event around every stage of a timed call.  Every
plan of the encoder must leave all of them recorded — a launcher that returned early would leave one out and profile_end
could not take its time — and timing must not change a byte of the output."""
import math

import numpy as np
import pytest
import torch

import alac_amd

pytestmark = pytest.mark.gpu

PACKETS = 64
# (options, channels, packets per segment)
CONFIGS = {
    "tiny": ({}, 2, 1),
    "latency": ({"narrow": 0}, 2, 1),
    "latency_unfolded": ({"narrow": 0, "fold": 0}, 2, 1),
    "stagewise": ({"fused": 0}, 2, 1),
    "throughput": ({"thru": 1}, 2, 1),  # the two class finals on two streams
    "encoder_lane": ({"encoder_lane": 1}, 2, 1),
    "fast_mode": ({"fast_mode": 1}, 2, 1),
    "overlapped_positions": ({}, 2, 4),  # 2 segments x 4 packets: the events are those of the last position
    "mono": ({}, 1, 1),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_every_stage_event_is_recorded(gpu_ctx, name):
    opts, channels, per = CONFIGS[name]
    n = PACKETS if per == 1 else 2 * per
    fmt = alac_amd.make_format(4096, 16, channels, 44100)
    pcm = torch.from_numpy(alac_amd.synth_pcm(0, n, fmt)).cuda()
    kw = {} if per == 1 else {"seg_first": torch.arange(0, n + 1, per, dtype=torch.int32).cuda()}
    with gpu_ctx.options(**opts):
        ref, ref_sizes = gpu_ctx.encode_to_host(fmt, pcm, n, **kw)
        gpu_ctx.profile_begin(2)
        got = [gpu_ctx.encode_to_host(fmt, pcm, n, **kw) for _ in range(2)]
        calls, stages = gpu_ctx.profile_end()
    print(name, calls, stages)
    assert calls == 2
    for stage, (ms, launches) in stages.items():
        assert math.isfinite(ms) and ms >= 0, (stage, ms)
        assert math.isfinite(launches) and launches >= 0, (stage, launches)
    assert stages["pack"][0] > 0 and stages["pack"][1] >= 1
    for stream, sizes in got:
        assert np.array_equal(sizes, ref_sizes)
        assert np.array_equal(stream, ref)
