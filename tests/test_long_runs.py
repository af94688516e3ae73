"""The 65 535-zero cap of the adaptive Golomb run code (ag_enc.c:333-349: a zero run is coded in 16 bits, so at 65 535
swallowed zeros the run is closed and zero mode is left; the decoder's counterpart is `nz >= 65535 -> zmode = 0`).
Every stage test elsewhere stops at 4096 residuals, so nothing there reaches it.  Here the oracle's dyn_comp /
dyn_decomp are pinned to the reference's compiled stages on zero runs around the first and second firing of the cap, live
where oracle/_ref is present, and through tests/golden/long_runs.npz (recipes + the reference's bytes and bit counts,
written by tests/golden/make_golden.py) everywhere.  tests/test_gpu_long_frames.py takes the GPU coders through the same
fixture."""
import numpy as np

from oracle_lib import LONG_RUN_BITS, LONG_RUN_PARAMS, coded_zero_runs, expand_recipe, load_long_runs, long_run_cases


def test_recipes_cover_the_cap():
    cases = long_run_cases()
    zeros = {int(rep) for c in cases for v, rep in c["recipe"] if v == 0}
    assert set(range(65533, 65539)) <= zeros and set(range(131070, 131074)) <= zeros and 200000 in zeros
    assert {c["bits"] for c in cases} == set(LONG_RUN_BITS)
    assert {(c["mb"], c["pb"], c["kb"]) for c in cases} == set(LONG_RUN_PARAMS)
    for key in ("bits", "mb"):  # both start bit offsets at every bit size and with either triple
        assert {(c[key], c["start_bit"]) for c in cases} == {(c[key], s) for c in cases for s in (0, 5)}
    first = [c["recipe"][0][0] == 0 for c in cases]
    last = [c["recipe"][-1][0] == 0 for c in cases]
    assert any(first) and any(last) and not all(first) and not all(last)


def test_oracle_matches_reference_objects_on_long_zero_runs(oracle, ref):
    for c in long_run_cases():
        pc = expand_recipe(c["recipe"])
        kw = dict(start_bit=c["start_bit"], mb0=c["mb"], pb=c["pb"], kb=c["kb"])
        d1, n1 = oracle.dyn_comp(pc, c["bits"], **kw)
        d2, n2 = oracle.dyn_comp(pc, c["bits"], fn=ref.lib.ref_dyn_comp_flat, **kw)
        assert n1 == n2 and np.array_equal(d1, d2), c
        st, back, n3 = oracle.dyn_decomp(d2, len(d2), len(pc), c["bits"], **kw)
        st2, back2, n4 = oracle.dyn_decomp(d1, len(d1), len(pc), c["bits"], fn=ref.lib.ref_dyn_decomp_flat, **kw)
        assert st == st2 == 0 and n3 == n4 == n1, c
        assert np.array_equal(back, pc) and np.array_equal(back2, pc), c


def test_fixture_holds_the_recipes():
    """the committed file was written from oracle_lib.long_run_cases as it stands"""
    fix, cases = load_long_runs(), long_run_cases()
    assert len(fix) == len(cases)
    for f, c in zip(fix, cases):
        assert np.array_equal(f["recipe"], np.asarray(c["recipe"]).reshape(-1, 2))
        assert (f["bits"], f["mb"], f["pb"], f["kb"], f["start_bit"]) == (c["bits"], c["mb"], c["pb"], c["kb"], c["start_bit"])
        assert f["n"] == int(np.asarray(c["recipe"])[:, 1].sum())


def test_oracle_reproduces_long_run_fixture(oracle):
    """the pin where the reference objects are absent: oracle == the bytes and bit counts the reference's dyn_comp gave, and
    the oracle's dyn_decomp reads them back"""
    nbits = {}
    for f in load_long_runs():
        pc = expand_recipe(f["recipe"])
        kw = dict(start_bit=f["start_bit"], mb0=f["mb"], pb=f["pb"], kb=f["kb"])
        data, n = oracle.dyn_comp(pc, f["bits"], **kw)
        assert n == f["nbits"] and np.array_equal(data, f["data"]), f["id"]
        st, back, n2 = oracle.dyn_decomp(f["data"], len(f["data"]), len(pc), f["bits"], **kw)
        assert st == 0 and n2 == n and np.array_equal(back, pc), f["id"]
        if len(f["recipe"]) == 1:
            nbits[(int(f["recipe"][0][1]), f["bits"], f["mb"])] = n
    # all-zero vectors of Z residuals: one ordinary symbol, then a run of Z - 1 zeros.  The run of 65 535 fills the 16-bit
    # count and is closed by the cap; one zero more is a symbol of its own behind it.
    for bits in LONG_RUN_BITS:
        assert nbits[(65535, bits, 10)] == nbits[(65536, bits, 10)] < nbits[(65537, bits, 10)], bits


def test_run_walker_on_closed_forms(oracle):
    """coded_zero_runs (what tests/test_gpu_long_frames.py proves its inputs with): Z zeros are one ordinary symbol, runs of
    65 535 each followed by one ordinary zero, and the rest; behind a large residual the mean first has to decay, one ordinary
    zero per step of mb -= (40 mb) >> 9 down to mb < 128 — and the bit count of the oracle's dyn_comp changes where the walk
    puts the cap"""
    for z, want in ((5, [(1, 4)]), (65535, [(1, 65534)]), (65536, [(1, 65535)]), (65537, [(1, 65535)]),
                    (65538, [(1, 65535), (65537, 1)]), (131073, [(1, 65535), (65537, 65535)]),
                    (131075, [(1, 65535), (65537, 65535), (131073, 2)])):
        assert coded_zero_runs(np.zeros(z, np.int32)) == want, z
    for first in (1, 7, 300, -300, 20000):
        mb, lead = 40 * (2 * abs(first) - (first < 0)) + 10, 0  # the mean behind the first symbol (mb0 = 10)
        while mb >= 128:
            mb, lead = mb - ((40 * mb) >> 9), lead + 1
        r = np.concatenate([[first], np.zeros(70000, np.int64), [3]]).astype(np.int32)
        assert coded_zero_runs(r) == [(1 + lead, 65535), (1 + lead + 65536, 70000 - lead - 65536)], first
        # the oracle agrees with where the walk puts the cap: below it the run is one 25-bit escape code whatever its length and
        # the symbol behind it is coded in zero mode; the run that reaches the cap leaves zero mode, so the same symbol codes
        # differently from exactly that length on
        at = lead + 65535
        bits = [oracle.dyn_comp(np.concatenate([[first], np.zeros(k, np.int64), [3]]).astype(np.int32), 16)[1]
                for k in (at - 3, at - 2, at - 1, at)]
        assert bits[0] == bits[1] == bits[2] != bits[3], (first, bits)
