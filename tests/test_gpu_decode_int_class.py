"""GPU: ALACDecoder::DecodeBatchInt (tests/cpp/decode_int.cpp).  On a two-packet 24-bit stereo stream with a short last
packet the class's integer decode must equal DecodeBatch's bytes unpacked on the host — planar int32 left-justified with a gap
behind each row, interleaved int32 right-justified, and packed 3-byte containers — and refuse containers narrower than the
stream."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_verify import encode_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def harness(gpu_ctx):
    subprocess.check_call(["make", "-C", CPP, "-f", "decode_int.mk", "decode_int"], stdout=subprocess.DEVNULL)
    return os.path.join(CPP, "decode_int")


def test_decode_batch_int_equals_decode_batch_unpacked(gpu_ctx, harness, tmp_path):
    frames = 4096 + 1000
    c = encode_case(gpu_ctx, 24, 2, frames, seed=71)
    assert c.n == 2
    (tmp_path / "cookie").write_bytes(c.cookie.tobytes())
    (tmp_path / "stream").write_bytes(c.stream.tobytes())
    (tmp_path / "sizes").write_bytes(c.sizes.astype(np.uint32).tobytes())
    p = subprocess.run([harness] + [str(tmp_path / n) for n in ("cookie", "stream", "sizes")], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.split() == ["ok", str(frames), str(3 * 2 * c.n * 4096)]
