"""lpc_ref.py — TEST INFRASTRUCTURE ONLY (imported by tests/ and tests/golden/make_golden.py, never by the product).

A host reference of the LPC encode mode's decision (alac_amd/csrc/alac_lpc.hip, k_lpc) for one packet, exact to the bit:

    planes        Forger.planes: the shift, then the u / v mix of Apple's independent packet (its mixRes, escape flag)
    r[0..30]      exact integers, r[L] = sum_{L <= j < N} x[j] x[j-L].  Every product and partial sum is an integer of
                  magnitude <= r[0] (Cauchy-Schwarz); asserted <= 2^53, the GPU's double sums are exact in any order
    Levinson      the loop of lpc_levinson in float64: the three steps the kernel writes as fma() are correctly rounded
                  fmas here (fma() below), division and product are Python's IEEE ones, rint rounds half to even
    drop rules    r[0] <= 0: no candidates; |k_m| >= 1 or err <= 0: stop; 2 m >= N: stop; den < 5: this candidate only;
                  den = the largest <= 15 with rint(amax 2^den) <= 32767
    costs         16 * order + the bits of the oracle's pc_block (general loop) and dyn_comp (pb * 4 / 4); Apple's channel
                  16 * num + bits with Apple's own parameters
    winner        strictly smaller cost wins; ties go to Apple's channel, then to the lower order

`decide` returns the winning ChannelParams per channel and a trace of every candidate; `stream` forges the whole LPC
stream of a file, so that its sizes and FNV can be computed without a GPU.
"""
from math import comb

import numpy as np

import forge

ORDERS = (4, 8, 12, 16, 24, 30)
MAX_ORDER = 30
EXACT = 1 << 53  # doubles hold every integer up to here


def fma(a, b, c):
    """a * b + c rounded once (IEEE fma, round to nearest even), on Python floats.  Every finite double is an integer over
    a power of two, so the exact value is one integer quotient, and int / int rounds correctly."""
    an, ad = a.as_integer_ratio()
    bn, bd = b.as_integer_ratio()
    cn, cd = c.as_integer_ratio()
    pn, pd = an * bn, ad * bd
    if pd >= cd:
        return (pn + cn * (pd // cd)) / pd
    return (pn * (cd // pd) + cn) / cd


def autocorr(x, n):
    """r[0..30] of the first n samples of plane x, exact Python integers"""
    x = np.asarray(x, np.int64)[:n]
    r0 = int(np.dot(x, x)) if n else 0
    assert r0 <= EXACT, f"r[0] = {r0} above 2^53: the kernel's double autocorrelation would round"
    return [r0] + [int(np.dot(x[L:], x[:n - L])) if n > L else 0 for L in range(1, MAX_ORDER + 1)]


class Cand:
    """one candidate of the trace: order, den (0 when not live), coefs (int list), cost (None when not live), drop reason
    (None when live): 'r0', 'k' (|k_m| >= 1), 'err' (error not positive), 'short' (2 m >= N), 'den' (den < 5)"""

    def __init__(self, order, drop=None, den=0, coefs=None):
        self.order, self.drop, self.den, self.coefs, self.cost = order, drop, den, coefs or [], None

    def __repr__(self):
        return f"Cand({self.order}, drop={self.drop}, den={self.den}, cost={self.cost})"


def levinson(r, n):
    """lpc_levinson's candidate table: [Cand] for every order of ORDERS, live or with the reason it was dropped"""
    out = []

    def stop(reason):
        out.extend(Cand(o, reason) for o in ORDERS[len(out):])
        return out

    r = [float(v) for v in r]  # exact (autocorr's bound)
    if not r[0] > 0.0:
        return stop("r0")
    a = [0.0] * (MAX_ORDER + 1)
    err = r[0]
    for m in range(1, MAX_ORDER + 1):
        if len(out) == len(ORDERS):
            break
        acc = r[m]
        for i in range(1, m):
            acc = fma(-a[i], r[m - i], acc)
        km = acc / err
        if not abs(km) < 1.0:
            return stop("k")
        t = [fma(-km, a[m - i], a[i]) for i in range(1, m)]
        a[1:m] = t
        a[m] = km
        err = err * fma(-km, km, 1.0)
        if not err > 0.0:
            return stop("err")
        if m != ORDERS[len(out)]:
            continue
        if 2 * m >= n:
            return stop("short")
        amax = max(abs(v) for v in a[1:m + 1])
        den = 15
        while den >= 5 and round(amax * (1 << den)) > 32767:
            den -= 1
        if den < 5:
            out.append(Cand(m, "den"))
            continue
        out.append(Cand(m, den=den, coefs=[round(v * (1 << den)) for v in a[1:m + 1]]))
    return out


def channel_bits(oracle, x, n, cp, chan_bits):
    """the bit count of one channel's residuals with header cp (mode 0): pc_block, then dyn_comp at pb * pbFactor / 4"""
    res, _ = oracle.pc_block(np.asarray(x, np.int32)[:n], n, cp.coefs, cp.num, chan_bits, cp.den_shift)
    return oracle.dyn_comp(res[:n], chan_bits, pb=40 * cp.pb_factor // 4)[1]


class Decision:
    """k_lpc's result for one packet: params [ChannelParams] (the winner per channel), winner [order, or None for Apple's
    channel], trace [[Cand]] per channel, apple_cost [int] per channel; escape / mix_bits / mix_res / shifted as Apple's"""

    def __init__(self, escape, shifted, mix_bits, mix_res):
        self.escape, self.shifted, self.mix_bits, self.mix_res = escape, shifted, mix_bits, mix_res
        self.params, self.winner, self.trace, self.apple_cost = [], [], [], []


def decide(oracle, pcm, n, depth, channels, apple_pkt):
    """k_lpc's decision for one packet of n sample-frames of packed PCM, given Apple's independent packet of the same PCM
    (oracle.encoder(...).encode_stream(..., segment_packets=1)): the mix decision, shift, escape flag and Apple's channel
    parameters come from its header"""
    escape, _, shifted, mix_bits, mix_res, apple = forge.parse_header(apple_pkt, channels)
    d = Decision(escape, shifted, mix_bits, mix_res)
    if escape or n == 0:
        return d
    planes, _, chan_bits = forge.Forger.planes(pcm, n, depth, channels, mix_bits, mix_res, shifted)
    for c in range(channels):
        ap = apple[c]
        best = 16 * ap.num + channel_bits(oracle, planes[c], n, ap, chan_bits)
        d.apple_cost.append(best)
        trace = levinson(autocorr(planes[c], n), n)
        win, wp = None, ap
        for cd in trace:
            if cd.drop:
                continue
            cp = forge.ChannelParams(num=cd.order, den_shift=cd.den, pb_factor=4, mode=0, coefs=cd.coefs)
            cd.cost = 16 * cd.order + channel_bits(oracle, planes[c], n, cp, chan_bits)
            if cd.cost < best:
                best, win, wp = cd.cost, cd.order, cp
        d.params.append(wp)
        d.winner.append(win)
        d.trace.append(trace)
    return d


def stream(oracle, pcm, total, depth, channels, frame_size, rate=44100):
    """the whole LPC stream of a file, forged on the host: (stream bytes, packet sizes, [Decision] per packet).  Packets
    where no candidate wins are Apple's independent packets, byte for byte; the others are forged with the winners."""
    enc = oracle.encoder(frame_size, depth, channels, rate)
    ind, isz = enc.encode_stream(pcm, total, segment_packets=1)
    bpf = channels * forge.BPS[depth]
    forger = forge.Forger(oracle)
    ends = np.cumsum(isz.astype(np.int64))
    out, decisions = [], []
    for p, (size, end) in enumerate(zip(isz.astype(np.int64), ends)):
        apple_pkt = ind[end - size:end]
        n = min(frame_size, total - p * frame_size)
        src = np.ascontiguousarray(pcm[p * frame_size * bpf:(p * frame_size + n) * bpf], np.uint8)
        d = decide(oracle, src, n, depth, channels, apple_pkt)
        decisions.append(d)
        if d.escape or all(w is None for w in d.winner):
            out.append(apple_pkt)
        else:
            out.append(forger.element(src, n, depth, channels, frame_size, d.params, mix_bits=d.mix_bits,
                                      mix_res=d.mix_res, bytes_shifted=d.shifted))
    sizes = np.array([len(b) for b in out], np.uint32)
    return (np.concatenate(out) if out else np.zeros(0, np.uint8)), sizes, decisions


# ---- edge signals ------------------------------------------------------------------------------------------------------

EDGE_KINDS = ("silence", "binomial", "window", "ar4", "ar8", "ar12", "ar16", "ar24", "ar30", "quiet", "noise", "ramp")


def _ar(rng, order, n, radius):
    """an AR(order) process of resonances (order / 2 pole pairs at `radius`, angles spread over (0, pi)), unit peak"""
    poly = np.array([1.0])
    for th in np.sort(rng.uniform(0.05, 3.0, order // 2)):
        poly = np.convolve(poly, [1.0, -2 * radius * np.cos(th), radius * radius])
    e = rng.standard_normal(n + 2000)
    y = np.zeros_like(e)
    for j in range(len(e)):  # y[j] = e[j] - sum poly[k] y[j-k]
        k = min(j, order)
        y[j] = e[j] - np.dot(poly[1:k + 1], y[j - 1::-1][:k]) if k else e[j]
    y = y[2000:]
    return y / np.abs(y).max()


def edge_plane(kind, n, bits, rng):
    """one plane of n samples in `bits` signed bits (the plane after the byte shift) that drives the search to one of its
    edges: r[0] = 0, a Levinson recursion that turns unstable (binomial: the data polynomial (1 - z)^K is nearly singular),
    den < 5 (binomial, window: smooth band-limited noise under a Hann^2 window), a winner at each order (arP), Apple's
    channel winning (quiet), escape (noise), den = 15 (ramp), a quiet tone (tone)"""
    A = (1 << (bits - 1)) - 1
    t = np.arange(n)
    if kind == "silence":
        return np.zeros(n, np.int64)
    if kind == "binomial":
        K = max(k for k in range(2, 25, 2) if comb(k, k // 2) <= A)
        b = np.array([comb(K, j) * (-1) ** j for j in range(K + 1)], np.int64) * (A // comb(K, K // 2))
        x = np.zeros(n, np.int64)
        at = min(int(rng.integers(0, 200)), max(n - K - 1, 0))
        x[at:at + K + 1] = b[:n - at]
        return x
    if kind == "window":
        X = np.fft.rfft(rng.standard_normal(n))
        X[int(0.6 * len(X)):] = 0
        x = np.fft.irfft(X, n) * (0.5 - 0.5 * np.cos(2 * np.pi * t / n)) ** 2
        return np.round(x / np.abs(x).max() * A).astype(np.int64)
    if kind.startswith("ar"):
        return np.round(_ar(rng, int(kind[2:]), n, 0.995) * A * 0.5).astype(np.int64)
    if kind == "quiet":
        return rng.integers(-3, 4, n)
    if kind == "noise":
        return rng.integers(-A - 1, A + 1, n)
    if kind == "ramp":
        return (t * 7 - n * 3) % (2 * A) - A
    if kind == "tone":
        return np.round((A >> 6) * np.sin(0.3 * t + 1)).astype(np.int64) + rng.integers(-2, 3, n)
    raise ValueError(kind)


def edge_signal(depth, channels, frame_size=4096, tail=20, seed=0):
    """packed PCM of one packet per EDGE_KIND and a partial last packet of `tail` frames (a quiet tone, so that it is
    compressed: orders with 2 * order >= tail stop the recursion), and its frame count.  Stereo: the channels of every other packet are one plane
    and its negation plus a little noise (the mix search takes mixRes != 0 there), the others independent planes."""
    rng = np.random.default_rng(seed * 1000 + depth * 10 + channels)
    shift = 8 * (2 if depth == 32 else 1 if depth >= 24 else 0)
    bits = depth - shift
    cols = []
    for p, kind in enumerate(EDGE_KINDS + ("tone",)):
        n = tail if p == len(EDGE_KINDS) else frame_size
        x = edge_plane(kind, n, bits, rng)
        if channels == 2:
            if p % 2:
                y = edge_plane(kind, n, bits, rng)
            else:
                y = np.clip(-x + rng.integers(-2, 3, n) * (kind != "silence"), -(1 << (bits - 1)), (1 << (bits - 1)) - 1)
            x = np.stack([x, y])
        else:
            x = x[None]
        if shift:
            x = (x << shift) | rng.integers(0, 1 << shift, x.shape)
        cols.append(x)
    x = np.concatenate(cols, axis=1)
    return forge.channels_to_pcm(x, depth), x.shape[1]


def paths(decisions):
    """the search paths a list of Decisions reached: drop reasons, 'den15' / 'den5..14' for live candidates, 'win<order>',
    'win_apple', 'mix0' / 'mix!=0' for non-escaped stereo packets, 'escape'"""
    seen = set()
    for d in decisions:
        if d.escape:
            seen.add("escape")
            continue
        if len(d.trace) == 2:
            seen.add("mix0" if d.mix_res == 0 else "mix!=0")
        for tr, w in zip(d.trace, d.winner):
            seen.add("win_apple" if w is None else f"win{w}")
            for cd in tr:
                seen.add(cd.drop or ("den15" if cd.den == 15 else "den5..14"))
    return seen
