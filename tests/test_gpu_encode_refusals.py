"""GPU: the refusals of the encode family's twelve entry points (encode, encode_segmented, encode_float, encode_float_dither,
encode_int, pcm_requantize and the six host forms) are the ones tests/golden/encode_refusals.json pins: same status, same
alac_hip_last_error text, in the same order of checks (each case breaks one argument of the accepted call, several cases
break two).  The list was recorded by tests/make_encode_refusals.py on the library of the commit in front of the one that
gave the family one source description and one call description; this file replays it on the library under test.

A refusal writes nothing: every output buffer, device and host, is filled with a sentinel byte in front of each call and must
still hold it afterwards.  The two exceptions are pinned too: a host form zeroes *out_total_bytes in front of its checks, and a
3-channel float call has zeroed its clip counters by the time it reads a segment table without a bound back."""
import json

import pytest

import make_encode_refusals as rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def replay(gpu_ctx):
    with open(rec.GOLDEN) as f:
        want = json.load(f)
    return want, rec.record(gpu_ctx)


def key(e):
    return (e["rig"], e["entry"], e["case"])


def test_same_calls_in_the_same_order(replay):
    want, got = replay
    assert [key(e) for e in got] == [key(e) for e in want]
    assert {e["entry"] for e in want if e["status"] < 0} == set(rec.PARAMS)
    assert {e["rig"] for e in want} == {r[0] for r in rec.RIGS}


def test_status_and_error_text(replay):
    want, got = replay
    diff = [(key(w), (w["status"], w["error"]), (g["status"], g["error"])) for w, g in zip(want, got)
            if (w["status"], w["error"]) != (g["status"], g["error"])]
    assert diff == []


def test_refusals_write_nothing(replay):
    want, got = replay
    diff = [(key(w), w["touched"], g["touched"]) for w, g in zip(want, got) if w["touched"] != g["touched"]]
    assert diff == []
    wrote = {key(g): g["touched"] for g in got if g["status"] < 0 and g["touched"]}
    assert all(v == rec.LATE.get(k, rec.EARLY) for k, v in wrote.items()), wrote
