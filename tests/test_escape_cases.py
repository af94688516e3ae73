"""The input builders of tests/test_gpu_escape_decisions.py, without a GPU: every search finds what the GPU tests claim to run,
the fallback tables NO_LATE_CASE / NO_TIE_CASE say exactly which formats a fresh search leaves empty (so they can neither grow
by accident nor hide a case), and the searches are deterministic and quick enough to run in every session."""
import time

import numpy as np

import test_gpu_escape_decisions as E


def test_late_table_is_what_a_fresh_search_gives(oracle):
    missing = []
    for depth, channels in E.FORMATS:
        for n in sorted(set(E.LATE_AT.values())):
            probe = E.Probe(oracle, 512, depth, channels)
            found = E.late_packet(probe, 100, n, channels, depth)
            assert probe.calls <= 4000  # "a bounded search: at most a few thousand oracle calls"
            if found is None:
                missing.append((depth, channels))
            else:
                d = found[1]
                assert d["decided"] == 2 and d["min_bits"] < d["escape_bits"] <= d["body"]
    assert sorted(set(missing)) == sorted(E.NO_LATE_CASE)


def test_tie_table_is_what_a_fresh_search_gives(oracle):
    missing = []
    for field, formats, step in (("body", E.TIE_FORMATS, 1), ("min_bits", E.ESTIMATE_TIE_FORMATS, 8)):
        for depth, channels, frame, n, fast in formats:
            probe = E.Probe(oracle, frame, depth, channels, fast=fast)
            found = E.tie_packets(probe, 7, n, channels, depth, field=field, step=step)
            assert probe.calls <= E.TIE_CALL_CAP + 84
            if sorted(found) != [-step, 0, step]:
                missing.append((depth, channels, frame, n, fast))
                continue
            for dist, (x, d) in found.items():
                again = probe(x)
                assert again[field] - again["escape_bits"] == dist and again == d
                escaped = again["decided"] != 0
                assert escaped == (dist >= 0) or (field == "min_bits" and dist < 0)  # below the estimate the written size decides
    assert sorted(missing) == sorted(E.NO_TIE_CASE)


def test_batches_hold_what_they_claim_and_build_quickly(oracle):
    t0 = time.perf_counter()
    for depth, channels in E.FORMATS:
        if (depth, channels) not in E.NO_LATE_CASE:
            E.assert_late_batch(E.late_batch(oracle, depth, channels))
    for depth, channels in ((16, 2), (20, 1)):
        E.assert_late_batch(E.late_batch(oracle, depth, channels, 4096))
    for frame in (256, 333, 4096):
        b = E.guard_batch(oracle, frame)
        assert all(b.decisions[p]["bitsU"] > E.guard_bits(frame, 20, 1) for p in b.guard_at)
    for field, formats in (("body", E.TIE_FORMATS), ("min_bits", E.ESTIMATE_TIE_FORMATS)):
        for f in formats:
            if f not in E.NO_TIE_CASE:
                E.assert_tie_batch(E.tie_batch(oracle, *f, field))
    for depth, channels in ((16, 2), (24, 2), (20, 1)):
        b = E.chained_batch(oracle, depth, channels)
        assert [b.kinds()[p] for p in (2, 7, 12)] == [2, 1, 0]
    for channels, depth in ((3, 20), (6, 16)):
        E.assert_multichannel_batch(E.multichannel_batch(oracle, channels, depth))
    assert time.perf_counter() - t0 < 20.0  # seconds on one core for every batch of the file (about 0.2 s where this was written)


def test_builders_are_deterministic(oracle):
    a = E.late_packet(E.Probe(oracle, 512, 16, 1), 100, 512, 1, 16)
    b = E.late_packet(E.Probe(oracle, 512, 16, 1), 100, 512, 1, 16)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    ta = E.tie_packets(E.Probe(oracle, 256, 16, 2), 7, 256, 2, 16)
    tb = E.tie_packets(E.Probe(oracle, 256, 16, 2), 7, 256, 2, 16)
    assert sorted(ta) == sorted(tb) and all(np.array_equal(ta[k][0], tb[k][0]) for k in ta)
