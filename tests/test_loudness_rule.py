"""CPU: the loudness rule of include/alac_hip.h.  The restatement (tests/loudness_ref.py) gives BS.1770-4's table at 48 kHz, the
known loudness of a full-scale sine and of two EBU Tech 3341 signals; the library's host-only helpers (alac_hip_loudness_filter,
alac_hip_loudness_rows, alac_hip_loudness_integrated) equal the restatement; hand-built rows exercise every branch of the
gate."""
import math

import numpy as np
import pytest

import alac_amd
import loudness_ref as lr

RATES = [8000, 16000, 22050, 44100, 48000, 88200, 96000, 192000, 384000, 8010]


def sine(freq, fs, seconds, dbfs, channels=1):
    t = np.arange(int(round(seconds * fs)), dtype=np.float64)
    x = 10.0 ** (dbfs / 20.0) * np.sin(2.0 * math.pi * freq * t / fs)
    return np.repeat(x[:, None], channels, axis=1)


def lufs_of(x, fs, weights=None):
    rows, _ = lr.measure(x, fs)
    return lr.integrated(rows, fs // 10, weights)


def test_coefficients_at_48k_are_the_table_of_bs1770():
    assert np.abs(lr.coefficients(48000) - np.array(lr.BS1770_48K)).max() <= 1e-14


@pytest.mark.parametrize("fs", RATES)
def test_library_filter_equals_the_restatement(fs):
    assert np.abs(alac_amd.loudness_filter(fs) - lr.coefficients(fs)).max() <= 1e-14


@pytest.mark.parametrize("fs", [0, 7990, 8001, 44101, 384010, 400000])
def test_library_refuses_other_rates(fs):
    lib = alac_amd.load_library()
    out = np.zeros(10)
    assert lib.alac_hip_loudness_filter(fs, out.ctypes.data) == -50
    assert lib.alac_hip_loudness_filter(48000, None) == -50
    assert lib.alac_hip_loudness_rows(fs, 100000, None, 1) == 0
    assert lib.alac_hip_loudness_workspace_bytes(fs, 2, 100000, 1) == 0


def test_full_scale_997_hz_sine_is_minus_3_01_lufs():
    v = lufs_of(sine(997.0, 48000, 2.0, 0.0), 48000)
    print("997 Hz 0 dBFS mono:", v)
    assert abs(v - (-3.01)) <= 0.01


def test_tech_3341_stereo_minus_23_dbfs_sine():
    v = lufs_of(sine(1000.0, 48000, 20.0, -23.0, channels=2), 48000)
    print("Tech 3341 case 1:", v)
    assert abs(v - (-23.0)) <= 0.1


def test_tech_3341_gated_sequence():
    """-36 / -23 / -36 dBFS for 10 s, 60 s and 10 s; here 2 s, 30 s and 2 s.  The quiet parts lie under the relative gate
    (-33) whatever their length.  What their length does not change either: three gating blocks straddle each step and pass
    the gate, with 0.7625, 0.525 and 0.2875 of the loud power.  Against the 297 loud blocks of 30 s they move the mean by
    10 log10((297 + 3.15) / 303) = -0.04 LU (-0.02 LU in the full sequence): the document's -23.0 +- 0.1 is kept."""
    fs = 48000
    x = np.concatenate([sine(1000.0, fs, 2.0, -36.0, 2), sine(1000.0, fs, 30.0, -23.0, 2), sine(1000.0, fs, 2.0, -36.0, 2)])
    v = lufs_of(x, fs)
    print("Tech 3341 case 3 (shortened):", v)
    assert abs(v - (-23.0)) <= 0.1


def rows_at(levels, hop, channels=1):
    """rows [len(levels), channels] whose every gating block of equal rows has the loudness `levels` names"""
    z = np.array([10.0 ** ((l + 0.691) / 10.0) if l is not None else 0.0 for l in levels])
    return np.repeat((z * hop)[:, None], channels, axis=1)


GATE_CASES = {
    "fewer than 4 rows": (rows_at([-20.0] * 3, 800), None),
    "exactly 4 rows": (rows_at([-20.0] * 4, 800), None),
    "no rows": (np.zeros((0, 2)), None),
    "all digital silence": (rows_at([None] * 12, 800, 2), None),
    "all under the absolute gate": (rows_at([-75.0] * 12, 800), None),
    "absolute gate drops the quiet part": (rows_at([-20.0] * 10 + [-80.0] * 10, 800), None),
    "relative gate drops the quiet part": (rows_at([-20.0] * 10 + [-35.0] * 10, 800), None),
    "relative gate keeps the near part": (rows_at([-20.0] * 10 + [-26.0] * 10, 800), None),
    "lfe carries no weight": (np.concatenate([rows_at([-30.0] * 8, 4800, 5), rows_at([0.0] * 8, 4800, 1)], axis=1), None),
    "lfe alone": (np.concatenate([np.zeros((8, 5)), rows_at([0.0] * 8, 4800, 1)], axis=1), None),
    "surround weight 1.41": (np.concatenate([np.zeros((8, 3)), rows_at([-20.0] * 8, 4800, 2)], axis=1), None),
    "8 channels": (rows_at([-20.0, -21.0, -19.0, -40.0, -18.0, -22.0, -20.0, -20.0], 4410, 8), None),
    "explicit weights": (rows_at([-20.0] * 8, 800, 3), [0.5, 0.0, 2.0]),
}


@pytest.mark.parametrize("name", sorted(GATE_CASES))
def test_library_gate_equals_the_restatement(name):
    rows, weights = GATE_CASES[name]
    hop = 4800 if rows.shape[1] >= 5 and name != "8 channels" else 4410 if name == "8 channels" else 800
    want = lr.integrated(rows, hop, weights)
    got = alac_amd.integrated_loudness(rows, hop, weights)
    print(name, want, got)
    if math.isinf(want):
        assert got == -math.inf
    else:
        assert abs(got - want) <= 1e-12


def test_the_gate_cases_take_the_branches_they_name():
    f = lambda name, hop=800: lr.integrated(GATE_CASES[name][0], hop, GATE_CASES[name][1])
    for name in ("fewer than 4 rows", "no rows", "all digital silence", "all under the absolute gate"):
        assert f(name) == -math.inf, name
    assert abs(f("exactly 4 rows") - (-20.0)) < 1e-9
    # 10 loud rows give 7 whole blocks; the three that straddle the step hold 3/4, 1/2 and 1/4 of the loud power plus the rest
    # of the quiet power q (relative to the loud one), and always pass; the 7 quiet blocks pass where they lie above both gates
    mean = lambda q, quiet_pass: (7 + 1.5 + 1.5 * q + (7 * q if quiet_pass else 0)) / (17 if quiet_pass else 10)
    assert abs(f("absolute gate drops the quiet part") - (-20.0 + 10.0 * math.log10(mean(1e-6, False)))) < 1e-9
    q = 10.0 ** -1.5
    assert -20.0 + 10.0 * math.log10(mean(q, True)) - 10.0 > -35.0  # the relative gate lies above the quiet part
    assert abs(f("relative gate drops the quiet part") - (-20.0 + 10.0 * math.log10(mean(q, False)))) < 1e-9
    assert abs(f("relative gate keeps the near part") - (-20.0 + 10.0 * math.log10(mean(10.0 ** -0.6, True)))) < 1e-9
    assert abs(f("lfe carries no weight", 4800) - (-30.0 + 10.0 * math.log10(1 + 1 + 1 + 1.41 + 1.41))) < 1e-9
    assert f("lfe alone", 4800) == -math.inf
    assert abs(f("surround weight 1.41", 4800) - (-20.0 + 10.0 * math.log10(2.82))) < 1e-9
    assert abs(f("explicit weights") - (-20.0 + 10.0 * math.log10(2.5))) < 1e-9


def test_library_gate_refusals():
    lib = alac_amd.load_library()
    import ctypes as C
    out = C.c_double(1.0)
    e = np.ones((8, 2))
    assert lib.alac_hip_loudness_integrated(e.ctypes.data, 8, 2, 800, None, None) == -50
    assert lib.alac_hip_loudness_integrated(None, 8, 2, 800, None, C.byref(out)) == -50
    assert lib.alac_hip_loudness_integrated(e.ctypes.data, 8, 0, 800, None, C.byref(out)) == -50
    assert lib.alac_hip_loudness_integrated(e.ctypes.data, 8, 9, 800, None, C.byref(out)) == -50
    assert lib.alac_hip_loudness_integrated(e.ctypes.data, 8, 2, 0, None, C.byref(out)) == -50
    assert out.value == 1.0
    assert lib.alac_hip_loudness_integrated(None, 0, 2, 800, None, C.byref(out)) == 0 and out.value == -math.inf


def test_row_count_equals_the_restatement():
    assert alac_amd.loudness_rows(8000, 10000) == 12
    assert alac_amd.loudness_rows(8000, 799) == 0
    table = [5, 5, 6, 805, 806, 1605, 4805, 4806]
    assert alac_amd.loudness_rows(8000, 5000, table) == sum((b - a) // 800 for a, b in zip(table, table[1:]))
    assert alac_amd.loudness_rows(8000, 4805, table) == 0  # ends behind total_frames
    assert alac_amd.loudness_rows(8000, 5000, [10, 5]) == 0
    for fs in RATES:
        L = lr.chunk_frames(fs)
        assert (fs // 10) % L == 0 and 16 <= L, (fs, L)
    assert [lr.chunk_frames(fs) for fs in (8000, 22050, 44100, 48000, 96000, 192000, 8010)] == \
        [50, 63, 63, 64, 64, 64, 89]


def test_scipy_lfilter_agrees_with_the_loop():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(5)
    for fs in (8000, 48000, 192000):
        x = rng.standard_normal((3000, 2)) * 0.3 + sine(25.0, fs, 3000 / fs, -1.0, 2)
        c = lr.coefficients(fs)
        y = signal.lfilter(c[5:8], np.r_[1.0, c[8:]], signal.lfilter(c[:3], np.r_[1.0, c[3:5]], x, axis=0), axis=0)
        ours = lr.kweight(x, fs)
        assert np.abs(y - ours).max() <= 1e-12 * max(1.0, np.abs(ours).max())
