"""The written coder's slot rule (alac_golomb.hpp golf_put / golf_open / golf_stream, enc_layout in alac_capi.hip).  The coder
makes no capacity test per symbol: once per 16-symbol block it pulls its word pointer back to 34 words before the end of its
slot of wcap words, and a stream that gets there "is longer than the escape size by itself, so nobody reads the slot".  Three
facts carry that comment; each is enumerated here from the symbol lengths of the oracle's dyn_comp (codec/ag_enc.c:115-184,
:249-367), restated in numpy:

  1. a symbol makes at most two puts of at most 32 bits (so a put completes at most one word);
  2. sixteen symbols plus the closing run code advance the pointer by at most 33 words (the word under assembly then sits at
     most at wcap - 1: inside the slot);
  3. for every depth, mono and stereo, frame sizes 1 .. 70 000 and every partial N: 32 (wcap - 34) + header >= escapeBits(N).

tests/test_gpu_escape_decisions.py drives streams past the guard on the GPU, where a short overrun of a mono slot would corrupt
nothing that is read; this file is the side that pins its absence."""
import numpy as np

KB, MAX_PREFIX, MAX_RUN_BITS, QB = 14, 9, 16, 512  # aglib.h:36-52
CHAN_BITS = range(9, 33)
ENCODER_CHAN_BITS = sorted({d - 8 * s + stereo for d, s in ((16, 0), (20, 0), (24, 1), (32, 2)) for stereo in (0, 1)})


def residual_puts(chan_bits):
    """every (k, quotient, remainder-is-zero) of dyn_code_32bit (ag_enc.c:151-184) -> the put lengths of the symbol, as the
    oracle writes it: one put of div + k + 1 - [mod == 0] bits, or the escape of MAX_PREFIX ones and chan_bits raw bits"""
    puts = [[MAX_PREFIX, chan_bits]]
    for k in range(1, KB + 1):
        for div in range(MAX_PREFIX):
            for de in (0, 1):
                bits = div + k + 1 - de
                puts.append([bits] if bits <= 25 else [MAX_PREFIX, chan_bits])
    return puts


def run_puts():
    """the zero-run code (dyn_code, ag_enc.c:115-148) for every mean that enters a run ((mb << 2) < QB, :328): k from :351"""
    out = []
    for mb in range(QB // 4):
        lead = 32 - int(mb).bit_length()
        k = lead - 24 + ((mb + 16) >> 6)
        assert 2 <= k <= 8  # golf_close_run: "k is 2..8 here", so & wb is the identity and the reciprocal table has the entry
        for div in range(MAX_PREFIX + 1):
            for de in (0, 1):
                out.append([min(div + k + 1 - de, MAX_PREFIX + MAX_RUN_BITS) if div < MAX_PREFIX else MAX_PREFIX + MAX_RUN_BITS])
    return out


def test_a_symbol_is_at_most_two_puts_of_at_most_32_bits():
    for cb in CHAN_BITS:
        for puts in residual_puts(cb) + run_puts():
            assert len(puts) <= 2 and max(puts) <= 32, (cb, puts)
    # golf_sym writes the escape as ONE put of 9 + chanBits bits ("requires bitSize <= 23"): every chanBits the encoder forms
    # (depth - shifted bytes + 1 for stereo) allows that, so a step of the lane-serial walk is a run code and a symbol: two puts
    assert ENCODER_CHAN_BITS == [16, 17, 20, 21] and all(MAX_PREFIX + cb <= 32 for cb in ENCODER_CHAN_BITS)
    assert max(max(p) for p in run_puts()) <= 25


def words_advanced(nacc, put_lengths):
    """golf_put's pointer arithmetic: nacc += nbits; wp += nacc >> 5; nacc &= 31"""
    words = 0
    for nbits in put_lengths:
        nacc += nbits
        words += nacc >> 5
        nacc &= 31
    return words


def test_sixteen_symbols_and_the_flush_advance_at_most_33_words():
    for cb in CHAN_BITS:
        fused = cb <= 23  # the GPU's one-put escape; beyond it the oracle's two puts
        worst_symbol = [MAX_PREFIX + cb] if fused else [MAX_PREFIX, cb]
        # a step closes a run (one put) and codes its residual; the block's last act is golf_finish: one more run code
        step = [MAX_PREFIX + MAX_RUN_BITS] + worst_symbol
        if fused:
            assert len(step) == 2
        for nacc in range(32):
            adv = words_advanced(nacc, step * 16 + [MAX_PREFIX + MAX_RUN_BITS])
            assert adv <= 16 * len(step) + 1  # a put completes at most one word
            if fused:
                assert adv <= 33, (cb, nacc, adv)
    # by count alone, whatever the lengths: 16 steps x 2 puts + 1 = 33 words from a pointer at most at wcap - 34 leaves the
    # word under assembly (stored by every put, and by golf_flush) at most at index wcap - 1
    assert 16 * 2 + 1 == 33 and (34 - 33) >= 1


def slot_words(frame, depth, channels):
    """wcap of enc_layout (alac_amd/csrc/alac_capi.hip:218-227), on arrays"""
    escape_bits = frame * depth * channels + 32 + 16
    wcap = ((escape_bits + 31) // 32 + 44 + 3) & ~3
    return wcap + (4 if depth == 24 else 0)


def escape_bits(n, frame, depth, channels):
    return n * depth * channels + np.where(n != frame, 32, 0) + 16  # codec/ALACEncoder.cu:459, :913


def smallest_header(n, frame, depth, channels):
    """what stands in a compressed element besides the written streams, with the fewest taps (4): 12 + 4 bits, the
    partial-frame word, mixBits / mixRes, per channel mode / denShift / pbFactor / numU and 4 coefficient words, and the
    shift-off bytes (ALACEncoder.cu:466-500, :919-938)"""
    shifted = 2 if depth == 32 else 1 if depth == 24 else 0
    return 16 + np.where(n != frame, 32, 0) + 16 + channels * (16 + 16 * 4) + n * 8 * shifted * channels


def test_a_stream_at_the_guard_is_past_the_escape_size():
    frames = np.arange(1, 70001, dtype=np.int64)
    for depth in (16, 20, 24, 32):
        for channels in (1, 2):
            wcap = slot_words(frames, depth, channels)
            assert (wcap % 4 == 0).all() and (wcap > 34).all()  # 16-byte aligned slots; the guard lies inside the slot
            guard = 32 * (wcap - 34)
            # escapeBits grows with N: the whole frame and the longest partial packet bound every N ...
            for n in (frames, np.maximum(frames - 1, 1)):
                assert (guard + smallest_header(n, frames, depth, channels) >= escape_bits(n, frames, depth, channels)).all()
                assert (guard >= escape_bits(n, frames, depth, channels)).all()  # (even without the header)
            # ... and every N outright, for the small frames and a few large ones
            for frame in list(range(1, 301)) + [333, 512, 4096, 65536, 70000]:
                n = np.arange(1, frame + 1, dtype=np.int64)
                g = 32 * (int(slot_words(frame, depth, channels)) - 34)
                assert (g + smallest_header(n, frame, depth, channels) >= escape_bits(n, frame, depth, channels)).all()
            # the lazy form (throughput regime) stops advancing when fewer than 4 of its wcap - 1 words are left: later still
            assert (32 * (wcap - 1 - 3 - 4) >= guard).all()

