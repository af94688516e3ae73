"""The encoder's SECOND escape decision, its size ties and the coder's slot guard.

An element escapes to uncompressed twice over (codec/ALACEncoder.cu): on the ESTIMATE (:455-461, minBits >= escapeBits, from
search passes that see only the first N / 8 samples) and LATE (:537-543 stereo, :952-958 mono: the element as written by the
final predictor + coder pass over all N samples is not smaller than the escape element, so it is rewound).  A late rewind
needs a packet whose first eighth looks compressible while the whole does not; no other generator of the suite builds one on
purpose.  The builders below do, each a short seeded search driven by the CPU oracle (oracle_lib's last_decision()):

  late    a cheap head of N / 8 + 8 samples, an expensive remainder;
  guard   20-bit mono late packets whose written stream (29 bits a sample against 20) runs past the coder's capacity guard,
          32 (wcap - 34) bits into its slot (alac_golomb.hpp golf_open; wcap from enc_layout, alac_capi.hip);
  tie     the written element within one bit of escapeBits (-1: kept, 0 and +1: rewound), reached by scaling the remainder
          and then nudging single samples behind the searched eighth by +-1..3 << e LSB of the coded part;
  estimate tie   minBits - escapeBits in {-8, 0, +8} (the estimate moves in steps of dilate = 8), by nudging head samples.

Every test first asserts ON THE CPU, from last_decision(), that its packets are of the kind it claims, then compares the GPU
stream byte for byte and size for size with the oracle's and decodes it back to the input with status 0.  A format for which a
search finds nothing goes into an asserted NO_*_CASE table (tests/test_escape_cases.py re-runs the searches without a GPU), never
into a skip.  The file carries its own option sets; it is not part of tests/test_gpu_variants.py's list.

LPC mode (option "lpc") has no case here: k_lpc (alac_lpc.hip) returns at once for a packet the ordinary encoder escaped, counts
every candidate exactly with lpc_pass<false> BEFORE it writes, and writes the winner only where its cost is below that of the
compressed channel it replaces — the written stream is shorter than one that did not escape, so it can neither reach the guard
nor change the escape decision."""
import functools

import numpy as np
import pytest

import alac_amd
from oracle_lib import channel_elements, interleave_channels

pytestmark = pytest.mark.gpu

OPTION_SETS = [{}, {"narrow": 0}, {"narrow": 0, "fold": 0}, {"thru": 1}, {"fused": 0}, {"encoder_lane": 1}, {"split_coder": 0},
               {"overlap_pos": 0}]
FEW_OPTION_SETS = [{}, {"narrow": 0}, {"thru": 1}, {"encoder_lane": 1}]
# alac_hip_encode_regime of these small batches under an option set, by the set's first key
REGIME_OF = {"default": "tiny", "narrow=0": "latency", "thru=1": "throughput", "fused=0": "stagewise", "encoder_lane=1": "lane",
             "split_coder=0": "tiny", "overlap_pos=0": "tiny"}
FORMATS = [(d, c) for d in (16, 20, 24, 32) for c in (1, 2)]  # (depth, channels)

# (depth, channels) for which the bounded search of late_packet() finds no late rewind at frame 512 — none: with a quiet head
# the 16-bit coded part of 16 / 24 / 32-bit mono stays ~100 bits short (full-scale noise costs ~16.4 bits a sample there), but
# the estimate only needs the head to cost less than 16 bits a sample, and a head of noise 12 bits wide in front of full-scale
# noise is rewound.  tests/test_escape_cases.py asserts this table against a fresh search.
NO_LATE_CASE = []
# (depth, channels, frame, N, fast) of TIE_FORMATS / ESTIMATE_TIE_FORMATS for which the search cannot bring the oracle to all
# three distances within 20 000 calls — none.
NO_TIE_CASE = []
TIE_FORMATS = [(16, 2, 256, 256, False), (24, 2, 256, 200, False), (20, 1, 256, 256, False), (32, 2, 512, 512, False),
               (16, 2, 256, 256, True)]  # the last: SetFastMode, which decides from the bits written (EncodeStereoFast)
ESTIMATE_TIE_FORMATS = [(16, 2, 256, 256, False), (16, 1, 256, 256, False)]
TIE_CALL_CAP = 20000


def id_of(opts):
    return ",".join(f"{k}={v}" for k, v in opts.items()) or "default"


def bytes_shifted(depth):
    return 2 if depth == 32 else 1 if depth == 24 else 0  # codec/ALACEncoder.cu:327-332


def slot_words(frame, depth, channels):
    """wcap of enc_layout (alac_amd/csrc/alac_capi.hip:218-227), restated: a channel's slot for its written bit string"""
    escape_bits = frame * depth * channels + 32 + 16
    wcap = ((escape_bits + 31) // 32 + 44 + 3) & ~3
    return wcap + 4 if depth == 24 else wcap


def guard_bits(frame, depth, channels):
    """the written coder pulls its word pointer back to slot + wcap - 34 once per 16 symbols (alac_golomb.hpp:104, :341)"""
    return 32 * (slot_words(frame, depth, channels) - 34)


def pack(x, depth):
    """[N][channels] integer samples -> packed little-endian interleaved PCM (20-bit samples sit in the top of 3 bytes)"""
    a = np.asarray(x, np.int64)
    if depth == 16:
        return a.astype("<i2").view(np.uint8).reshape(-1).copy()
    if depth == 32:
        return a.astype("<i4").view(np.uint8).reshape(-1).copy()
    if depth == 20:
        a = a << 4
    return (a & 0xffffff).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1).copy()


class Probe:
    """one oracle encoder per format, reset before every packet: what would this packet do as the first of a segment?"""

    def __init__(self, oracle, frame, depth, channels, fast=False):
        self.enc = oracle.encoder(frame, depth, channels, fast=fast)
        self.depth, self.calls = depth, 0

    def __call__(self, x):
        self.enc.reset()
        self.calls += 1
        self.enc.encode_packet(pack(x, self.depth), len(x))
        d = self.enc.last_decision()
        d["bitsU"] = self.enc.last_info()["bitsU"]
        return d


# ---- input builders ----------------------------------------------------------------------------------------------------------

def full_scale(rng, n, channels, depth):
    return rng.integers(-(1 << (depth - 1)), 1 << (depth - 1), (n, channels))


def quiet_tone(rng, n, channels, depth):
    """a sine an eighth of full scale with a little noise: compresses, and moves the coefficient rows"""
    t = np.arange(n)[:, None]
    amp = float(1 << (depth - 4))
    x = amp * np.sin(2 * np.pi * rng.uniform(200, 2000, channels) * t / 44100.0 + rng.uniform(0, 6, channels))
    return np.round(x + rng.standard_normal((n, channels)) * amp * 0.002).astype(np.int64)


def late_packet(probe, seed, n, channels, depth, want_guard=0):
    """A packet the oracle rewinds late (and whose written stream is longer than want_guard bits), or None.  First the plain
    form — quiet head of n / 8 + 8 samples, full-scale noise behind it; then, bounded, louder and shorter heads (the estimate
    only needs the head to cost less than the escape size per sample) in front of noise or full-scale values of random sign,
    and a spike train for the shortest packets."""
    unit = 1 << (8 * bytes_shifted(depth))
    hi, lo = (1 << (depth - 1)) - 1, -(1 << (depth - 1))
    forms = [(n // 8 + 8, 2, "noise")] + [(h, amp, tail) for amp in (12, 10, 13, 8) for h in (n // 8 + 8, n // 8)
                                          for tail in ("noise", "sign")] + \
        [(h, 2, "spikes") for h in (n // 8 + 8, n // 8, n // 8 + 1)]
    for attempt in range(4):
        for head, amp, tail in forms:
            head = min(head, n)
            rng = np.random.default_rng([seed, attempt, head, amp])
            x = full_scale(rng, n, channels, depth)
            if tail == "sign":
                x = np.where(x < 0, lo, hi)
            elif tail == "spikes":  # full-scale spikes of alternating sign, every other sample
                x[:] = 0
                x[0::4], x[2::4] = hi, lo
            x[:head] = rng.integers(-3, 4, (head, channels)) if amp == 2 else \
                rng.integers(-(1 << amp), (1 << amp) + 1, (head, channels)) * unit
            d = probe(x)
            if d["decided"] == 2 and d["bitsU"] > want_guard:
                return x, d
    return None


def tie_packets(probe, seed, n, channels, depth, field="body", step=1, cap=TIE_CALL_CAP):
    """{-step, 0, +step: (packet, decision)} with decision[field] - escape_bits at that distance; a distance not reached within
    `cap` oracle calls is missing.  field "body": quiet head, the remainder scaled by bisection until the written element
    straddles the escape size, then single samples BEHIND the searched eighth nudged by +-1..3 << e in units of the coded part's LSB (they
    cannot change the estimate, mixRes, numU or numV).  field "min_bits": the whole packet is noise, scaled until the ESTIMATE
    straddles the escape size, and the nudged samples are those of the searched eighth."""
    rng = np.random.default_rng([seed, n, channels, depth])
    unit = 1 << (8 * bytes_shifted(depth))
    coded = depth - 8 * bytes_shifted(depth)
    hi, lo = (1 << (depth - 1)) - 1, -(1 << (depth - 1))
    head = min(n // 8 + 8, n) if field == "body" else 0
    first, last = (head, n) if field == "body" else (0, n // 8)  # the samples that may be nudged
    noise = rng.integers(-(1 << (coded - 1)), 1 << (coded - 1), (n - head, channels))
    low = rng.integers(0, unit, (n - head, channels))
    quiet = rng.integers(-3, 4, (head, channels))
    start = probe.calls

    def scaled(s):
        return np.concatenate([quiet, np.round(noise * s).astype(np.int64) * unit + low])

    def dist(x):
        d = probe(x)
        if field == "body" and d["body"] == 0:
            return None, d  # the final pass did not run (never with a quiet head)
        return d[field] - d["escape_bits"], d

    a, b = 0.0, 1.0
    if dist(scaled(b))[0] is None or dist(scaled(b))[0] < 0 or dist(scaled(a))[0] >= 0:
        return {}
    for _ in range(40):
        m = 0.5 * (a + b)
        a, b = (a, m) if dist(scaled(m))[0] >= 0 else (m, b)
    x = scaled(b)
    cur, dec = dist(x)
    found = {}
    for target in (0, -step, step):
        while cur != target and probe.calls - start < cap:
            y = x.copy()
            i, c = int(rng.integers(first, last)), int(rng.integers(0, channels))
            # (1..3 LSB alone rarely move a symbol of k = 13 or 14 across a length boundary: the exponent spreads the nudges)
            nudge = int(rng.choice([-3, -2, -1, 1, 2, 3])) << int(rng.integers(0, coded - 3))
            y[i, c] = min(hi, max(lo, y[i, c] + nudge * unit))
            got, d = dist(y)
            if got is not None and abs(got - target) <= abs(cur - target):
                x, cur, dec = y, got, d
        if cur == target:
            found[target] = (x.copy(), dec)
    return found


# ---- batches: PCM + what the oracle makes of it, built once per format --------------------------------------------------------

class Batch:
    """packets (a list of [N][channels] sample arrays) of one format, in segments; the oracle's packets and segment states"""

    def __init__(self, oracle, frame, depth, channels, packets, seg_first=None, fast=False):
        self.frame, self.depth, self.channels, self.fast = frame, depth, channels, fast
        self.fmt = alac_amd.make_format(frame, depth, channels)
        self.n = len(packets)
        self.ns = np.array([len(x) for x in packets], np.int32)
        self.seg_first = None if seg_first is None else np.asarray(seg_first, np.int32)
        self.pcm = np.zeros(self.n * self.fmt.packet_bytes, np.uint8)
        self.src = [pack(x, depth) for x in packets]
        for p, s in enumerate(self.src):
            self.pcm[p * self.fmt.packet_bytes:p * self.fmt.packet_bytes + len(s)] = s
        enc = oracle.encoder(frame, depth, channels, fast=fast)
        bounds = list(range(self.n + 1)) if seg_first is None else list(seg_first)
        self.ref, self.decisions, self.states = [], [], []
        for a, b in zip(bounds[:-1], bounds[1:]):
            enc.reset()
            for p in range(a, b):
                self.ref.append(enc.encode_packet(self.src[p], int(self.ns[p])))
                self.decisions.append(dict(enc.last_decision(), bitsU=enc.last_info()["bitsU"]))
            self.states.append(enc.get_state())

    def kinds(self):
        return [d["decided"] for d in self.decisions]


def check_on_gpu(ctx, batch, opts):
    """the GPU's stream, sizes (and, for chained segments, final states) against the oracle's; decode back to the input"""
    import torch
    b = batch
    state = None
    kw = dict(num_samples=torch.from_numpy(b.ns).cuda())
    if b.seg_first is not None:
        state = torch.zeros((len(b.seg_first) - 1, 64), dtype=torch.int16).cuda()
        kw.update(seg_first=torch.from_numpy(b.seg_first).cuda(), state=state)
    first_key = id_of(opts).split(",")[0]
    if b.fast:
        opts = dict(opts, fast_mode=1)
    with ctx.options(**opts):
        # the option set really selects the kernels it is here for
        want = "tiny" if b.fast and b.channels == 2 and "encoder_lane" in opts else REGIME_OF[first_key]
        assert ctx.regime(b.fmt, b.n if b.seg_first is None else len(b.seg_first) - 1) == want, opts
        stream, sizes = ctx.encode_to_host(b.fmt, torch.from_numpy(b.pcm).cuda(), b.n, **kw)
    off = 0
    for p, want in enumerate(b.ref):
        assert sizes[p] == len(want), (opts, p, int(b.ns[p]), b.decisions[p])
        assert np.array_equal(stream[off:off + len(want)], want), (opts, p, int(b.ns[p]), b.decisions[p])
        off += len(want)
    assert off == len(stream)
    if state is not None and b.channels <= 2:
        got = state.cpu().numpy()
        for s, want in enumerate(b.states):
            assert np.array_equal(got[s], want), (opts, "state of segment", s)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])).cuda()
    out, dns, st, _ = ctx.decode(ctx.magic_cookie(b.fmt), torch.from_numpy(stream).cuda(), offs, b.n)
    ctx.synchronize()
    assert int(st.abs().sum()) == 0 and np.array_equal(dns.cpu().numpy(), b.ns)
    got = out.cpu().numpy()
    for p, s in enumerate(b.src):
        assert np.array_equal(got[p * b.fmt.packet_bytes:p * b.fmt.packet_bytes + len(s)], s), (opts, p)


LATE_AT = {0: 512, 1: 511, 11: 200, 12: 65, 23: 512}  # position -> samples: partial packets, so every running byte offset occurs
NOISE_AT = (5, 17)


@functools.lru_cache(maxsize=None)
def late_batch(oracle, depth, channels, frame=512):
    """24 packets (6 at frame 4096): late rewinds first, second, back to back in the middle and last, full-scale noise (escapes
    on the estimate) at two places, a quiet tone everywhere else"""
    probe = Probe(oracle, frame, depth, channels)
    rng = np.random.default_rng([depth, channels, frame])
    if frame == 512:
        late_at, noise_at, count = LATE_AT, NOISE_AT, 24
    else:
        late_at, noise_at, count = {0: frame, 2: frame - 1, 3: frame, 5: frame // 2 + 1}, (4,), 6
    packets = []
    for p in range(count):
        if p in late_at:
            found = late_packet(probe, 100 + p, late_at[p], channels, depth)
            assert found is not None, (depth, channels, frame, late_at[p])
            packets.append(found[0])
        elif p in noise_at:
            packets.append(full_scale(rng, frame, channels, depth))
        else:
            packets.append(quiet_tone(rng, frame, channels, depth))
    b = Batch(oracle, frame, depth, channels, packets)
    b.late_at, b.noise_at = late_at, noise_at
    return b


@functools.lru_cache(maxsize=None)
def guard_batch(oracle, frame):
    """20-bit mono: a guard-reaching packet first, between two compressed ones, as a partial packet, and last — next to the spare
    slot behind the batch's slots, where lanes without a packet dump their words"""
    probe = Probe(oracle, frame, 20, 1)
    rng = np.random.default_rng(frame)
    guard_at = {0: frame, 2: frame, 4: frame - 1, 6: frame}
    packets = []
    for p in range(7):
        if p in guard_at:
            found = late_packet(probe, 200 + p, guard_at[p], 1, 20, want_guard=guard_bits(frame, 20, 1))
            assert found is not None, (frame, p)
            packets.append(found[0])
        else:
            packets.append(quiet_tone(rng, frame, 1, 20))
    b = Batch(oracle, frame, 20, 1, packets)
    b.guard_at = guard_at
    return b


@functools.lru_cache(maxsize=None)
def tie_cases(oracle, depth, channels, frame, n, fast, field):
    probe = Probe(oracle, frame, depth, channels, fast=fast)
    found = tie_packets(probe, 7, n, channels, depth, field=field, step=1 if field == "body" else 8)
    return found, probe.calls


@functools.lru_cache(maxsize=None)
def tie_batch(oracle, depth, channels, frame, n, fast, field):
    """the tie packets at -step, 0, +step, each between compressed neighbours"""
    found, _ = tie_cases(oracle, depth, channels, frame, n, fast, field)
    rng = np.random.default_rng([depth, channels, frame, n])
    packets, tie_at = [quiet_tone(rng, frame, channels, depth)], {}
    for dist in sorted(found):
        tie_at[len(packets)] = dist
        packets += [found[dist][0], quiet_tone(rng, frame, channels, depth)]
    b = Batch(oracle, frame, depth, channels, packets, fast=fast)
    b.tie_at, b.field = tie_at, field
    return b


@functools.lru_cache(maxsize=None)
def chained_batch(oracle, depth, channels, frame=512):
    """three segments of five packets: packet 2 is rewound late in the first, escapes on the estimate in the second, compresses
    in the third; packets 3 and 4 hold the same PCM in all three, so they differ only through the coefficient rows packet 2 left"""
    probe = Probe(oracle, frame, depth, channels)
    rng = np.random.default_rng([9, depth, channels])
    lead = [quiet_tone(rng, frame, channels, depth) for _ in range(2)]
    trail = [quiet_tone(rng, frame, channels, depth) for _ in range(2)]
    late = late_packet(probe, 300, frame, channels, depth)
    assert late is not None
    middles = [late[0], full_scale(rng, frame, channels, depth), quiet_tone(rng, frame, channels, depth)]
    packets = []
    for mid in middles:
        packets += lead + [mid] + trail
    b = Batch(oracle, frame, depth, channels, packets, seg_first=[0, 5, 10, 15])
    # the same head (so the same searches, on the same rows) in front of another expensive remainder: what differs afterwards
    # was left by the final pass alone
    other = late[0].copy()
    other[frame // 8 + 8:] = full_scale(np.random.default_rng(301), frame - frame // 8 - 8, channels, depth)
    b.other_late = other
    return b


@functools.lru_cache(maxsize=None)
def multichannel_batch(oracle, channels, depth, frame=512):
    """3 channels: the mono element late; 6 channels: the first pair late — in packets 1, 3 (partial) and 5, the other elements
    (and the other packets) a quiet tone"""
    elements = channel_elements(oracle, channels)
    target = next(k for k, (ci, ech) in enumerate(elements) if ech == (1 if channels == 3 else 2))
    rng = np.random.default_rng([channels, depth])
    ns = [frame, frame, frame, 200, frame, frame, 333]
    late_in = (1, 3, 5)
    packets, kinds = [], []
    for p, n in enumerate(ns):
        parts, row = [], []
        for k, (ci, ech) in enumerate(elements):
            probe = Probe(oracle, frame, depth, ech)
            if p in late_in and k == target:
                x, d = late_packet(probe, 400 + p, n, ech, depth)
            else:
                x = quiet_tone(rng, n, ech, depth)
                d = probe(x)
            parts.append((pack(x, depth), ech))
            row.append(d["decided"])
        packets.append(interleave_channels(parts, depth))
        kinds.append(row)
    b = Batch.__new__(Batch)
    b.frame, b.depth, b.channels, b.fast = frame, depth, channels, False
    b.fmt = alac_amd.make_format(frame, depth, channels)
    b.n, b.ns, b.seg_first, b.src = len(ns), np.array(ns, np.int32), None, packets
    b.pcm = np.zeros(b.n * b.fmt.packet_bytes, np.uint8)
    enc = oracle.encoder(frame, depth, channels)
    b.ref, b.decisions = [], []
    for p, s in enumerate(packets):
        b.pcm[p * b.fmt.packet_bytes:p * b.fmt.packet_bytes + len(s)] = s
        enc.reset()
        b.ref.append(enc.encode_packet(s, ns[p]))
        b.decisions.append(enc.last_decision())
    b.element_kinds, b.target, b.late_in = kinds, target, late_in
    return b


# ---- the tests ----------------------------------------------------------------------------------------------------------------

def test_inventory(oracle, capsys):
    """what the builders found, per format (printed), and that nothing is missing that is not in a NO_*_CASE table"""
    lines, late, guard, ties = [], 0, 0, 0
    for depth, channels in FORMATS:
        if (depth, channels) in NO_LATE_CASE:
            continue
        b = late_batch(oracle, depth, channels)
        k = b.kinds().count(2)
        late += k
        lines.append(f"late   {depth:2d}-bit x{channels} frame 512: {k} packets, N = {sorted(set(b.late_at.values()))}")
    for frame in (256, 333, 4096):
        b = guard_batch(oracle, frame)
        over = [b.decisions[p]["bitsU"] - guard_bits(frame, 20, 1) for p in b.guard_at]
        guard += len(over)
        lines.append(f"guard  20-bit x1 frame {frame}: {len(over)} packets, {min(over)}..{max(over)} bits past the guard")
    for field, formats in (("body", TIE_FORMATS), ("min_bits", ESTIMATE_TIE_FORMATS)):
        for depth, channels, frame, n, fast in formats:
            if (depth, channels, frame, n, fast) in NO_TIE_CASE:
                continue
            found, calls = tie_cases(oracle, depth, channels, frame, n, fast, field)
            ties += len(found)
            lines.append(f"tie    {field:8s} {depth:2d}-bit x{channels} frame {frame} N {n}{' fast' if fast else ''}: "
                         f"{sorted(found)} after {calls} oracle calls")
    lines.append(f"total: {late} late, {guard} guard, {ties} tie packets; NO_LATE_CASE {len(NO_LATE_CASE)}, "
                 f"NO_TIE_CASE {len(NO_TIE_CASE)} formats")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert late == 5 * (len(FORMATS) - len(NO_LATE_CASE)) and guard == 12
    assert ties == 3 * (len(TIE_FORMATS) + len(ESTIMATE_TIE_FORMATS) - len(NO_TIE_CASE))


def assert_late_batch(b):
    kinds = b.kinds()
    for p, k in enumerate(kinds):
        want = 2 if p in b.late_at else 1 if p in b.noise_at else 0
        assert k == want, (b.depth, b.channels, p, b.decisions[p])
        if want == 2:  # escape == 1 and bitsU > 0 in last_info(): the final pass ran, then the element was rewound
            assert b.decisions[p]["body"] >= b.decisions[p]["escape_bits"] > b.decisions[p]["min_bits"]


@pytest.mark.parametrize("opts", OPTION_SETS, ids=id_of)
@pytest.mark.parametrize("depth,channels", [f for f in FORMATS if f not in NO_LATE_CASE])
def test_late_rewind_among_compressed_neighbours(gpu_ctx, oracle, depth, channels, opts):
    b = late_batch(oracle, depth, channels)
    assert_late_batch(b)
    check_on_gpu(gpu_ctx, b, opts)


@pytest.mark.parametrize("opts", OPTION_SETS, ids=id_of)
@pytest.mark.parametrize("depth,channels", [(16, 2), (20, 1)])
def test_late_rewind_after_many_tiles(gpu_ctx, oracle, depth, channels, opts):
    """frame 4096: the final pass crosses many tiles (and, for 20-bit mono, the slot guard) before the decision"""
    b = late_batch(oracle, depth, channels, 4096)
    assert_late_batch(b)
    check_on_gpu(gpu_ctx, b, opts)


@pytest.mark.parametrize("opts", OPTION_SETS, ids=id_of)
@pytest.mark.parametrize("frame", [256, 333, 4096])
def test_guard_reaching_streams(gpu_ctx, oracle, frame, opts):
    """Written streams go to per-channel slots of wcap words and the coder makes no per-symbol bound check; its four capacity
    mechanisms (golf_stream's pull-back to wcap - 34 once per 16 symbols, the lazy form's wleft, the first-generation coder's
    widx < wcap, k_splice_split's clamp of lenA + lenB) all rest on one claim: a stream that gets there is longer than the escape
    size by itself, so the packet escapes and nobody reads the slot.  Only 20-bit mono can get there (29 bits a sample against
    20).  With the split coder lenA + lenB exceeds the slot while neither half reaches its own guard.

    What this can see: the decision, the size and the bytes of the guard-reaching packet and of every neighbour — with such a
    packet first, last (next to the spare dump slot), between compressed packets and partial.  What it cannot: in mono the
    second slot of a packet is unused, so an overrun of less than one slot corrupts nothing that is read; the absence of a short
    overrun is pinned by the arithmetic of tests/test_coder_slot_rule.py, not here."""
    b = guard_batch(oracle, frame)
    limit = guard_bits(frame, 20, 1)
    assert limit == {256: 5568, 333: 7104, 4096: 82368}[frame]
    for p, d in enumerate(b.decisions):
        if p in b.guard_at:
            assert d["decided"] == 2 and d["bitsU"] > limit, (frame, p, d)  # the stream alone, without the element's header
        else:
            assert d["decided"] == 0, (frame, p, d)
    check_on_gpu(gpu_ctx, b, opts)


def assert_tie_batch(b):
    assert sorted(b.tie_at.values()) == ([-1, 0, 1] if b.field == "body" else [-8, 0, 8])
    for p, d in enumerate(b.decisions):
        if p not in b.tie_at:
            assert d["decided"] == 0, (p, d)
            continue
        assert d[b.field] - d["escape_bits"] == b.tie_at[p], (p, d)
        if b.field == "min_bits":
            assert (d["decided"] == 1) == (b.tie_at[p] >= 0), (p, d)  # both decisions are >=
        elif b.fast:  # EncodeStereoFast's estimate IS the written size (header included): it escapes there
            assert d["min_bits"] == d["body"] and d["decided"] == (1 if b.tie_at[p] >= 0 else 0), (p, d)
        else:
            assert d["decided"] == (2 if b.tie_at[p] >= 0 else 0), (p, d)


@pytest.mark.parametrize("opts", FEW_OPTION_SETS, ids=id_of)
@pytest.mark.parametrize("depth,channels,frame,n,fast", [f for f in TIE_FORMATS if f not in NO_TIE_CASE])
def test_size_ties(gpu_ctx, oracle, depth, channels, frame, n, fast, opts):
    """the written element one bit below, at and one bit above the escape size: a `>` for the `>=`, or one bit too many or too
    few in the body (header, shift-off bytes, coefficient words, the partial-frame word) changes a packet here"""
    b = tie_batch(oracle, depth, channels, frame, n, fast, "body")
    assert_tie_batch(b)
    check_on_gpu(gpu_ctx, b, opts)


@pytest.mark.parametrize("opts", FEW_OPTION_SETS, ids=id_of)
@pytest.mark.parametrize("depth,channels,frame,n,fast", [f for f in ESTIMATE_TIE_FORMATS if f not in NO_TIE_CASE])
def test_estimate_ties(gpu_ctx, oracle, depth, channels, frame, n, fast, opts):
    """minBits one step (dilate = 8 bits) below, at and one step above escapeBits"""
    b = tie_batch(oracle, depth, channels, frame, n, fast, "min_bits")
    assert_tie_batch(b)
    check_on_gpu(gpu_ctx, b, opts)


@pytest.mark.parametrize("opts", FEW_OPTION_SETS, ids=id_of)
@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (20, 1)])
def test_chained_segment_through_a_late_rewind(gpu_ctx, oracle, depth, channels, opts):
    """The final pass has adapted the coefficient row by the time the element is rewound, so the next packet of the segment
    starts from another row than after an estimate escape.  On the CPU: the packets behind the late rewind differ from those
    behind the estimate escape, and two late packets with the same head (same searches) but different remainders leave different
    rows — the final pass's adaptation is visible.  On the GPU: stream and state out equal the oracle's."""
    b = chained_batch(oracle, depth, channels)
    assert [b.kinds()[p] for p in (2, 7, 12)] == [2, 1, 0], b.kinds()
    assert all(k == 0 for p, k in enumerate(b.kinds()) if p % 5 != 2)
    assert not np.array_equal(b.ref[3], b.ref[8]) and not np.array_equal(b.states[0], b.states[1])
    enc = oracle.encoder(b.frame, depth, channels)
    rows = []
    for mid in (b.src[2], pack(b.other_late, depth)):
        enc.reset()
        for s in (b.src[0], b.src[1], mid):
            enc.encode_packet(s, b.frame)
        assert enc.last_decision()["decided"] == 2
        rows.append(enc.get_state())
    assert not np.array_equal(rows[0], rows[1])
    check_on_gpu(gpu_ctx, b, opts)


def assert_multichannel_batch(b):
    for p, row in enumerate(b.element_kinds):
        assert row == [2 if (p in b.late_in and k == b.target) else 0 for k in range(len(row))], (p, row)


@pytest.mark.parametrize("opts", FEW_OPTION_SETS, ids=id_of)
@pytest.mark.parametrize("channels,depth", [(3, 20), (6, 16)])
def test_multichannel_element_escapes_late(gpu_ctx, oracle, channels, depth, opts):
    """one element of a packet is rewound late while the others compress (each element classified by the oracle on its own)"""
    b = multichannel_batch(oracle, channels, depth)
    assert_multichannel_batch(b)
    check_on_gpu(gpu_ctx, b, opts)


def test_fast_mode_keeps_its_bytes_under_encoder_lane(gpu_ctx):
    """The first-generation encoder has no search-free form (found by test_size_ties: with both options set it used to run the
    searched encode).  A 2-channel stream in fast mode runs on the tap-parallel pipeline whatever "encoder_lane" says, and
    alac_hip_encode_regime says so; mono and 3..8-channel streams, which SetFastMode does not touch, stay on the lane kernel."""
    with gpu_ctx.options(fast_mode=1, encoder_lane=1):
        assert gpu_ctx.regime(alac_amd.make_format(256, 16, 2), 7) == "tiny"
        assert gpu_ctx.regime(alac_amd.make_format(256, 16, 1), 7) == "lane"
        assert gpu_ctx.regime(alac_amd.make_format(256, 16, 6), 7) == "lane"
    with gpu_ctx.options(encoder_lane=1):
        assert gpu_ctx.regime(alac_amd.make_format(256, 16, 2), 7) == "lane"
