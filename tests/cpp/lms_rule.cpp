// The threshold form of the predictor's coefficient update (lms_adapt_thresholds, alac_amd/csrc/alac_lms.hpp, compiled here
// for the host) against the early-exit walk of the oracle's unpc_block, one regular step at a time: a residual row of
// na + 2 samples whose na + 1 warm-up positions set up a chosen history and whose last sample is the chosen residual.
//
//   form    lane                               taps na      denShift  chanBits
//   any     8 slots, masks and weights by na   1 .. 8       1 .. 15   9 .. 23    lms_step_dec_any
//   wide    na slots, weights na - i           4, 8         9         9 .. 23    lms_step_dec_wide
//   pair    4 slots: na 4; 8 slots: na 4 | 8   4, 8         9         9 .. 23    lms_step_dec_pair
//   NOT covered: the two-lane step lms4_step_dec and the encoder's lms_step, which keep their own copies.
//   NOT covered: chanBits > 23.  A difference of two samples then has more than 24 bits, the 24-bit products are no
//   longer exact and a threshold can wrap; such chains take the generic walk (lms_adapt, alac_dev.hpp), never this rule.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "alac_lms.hpp"
#include "alac_oracle.h"

using alacdev::lms_adapt_thresholds;

static uint64_t rngState = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    rngState = rngState * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rngState >> 33);
}
static int32_t rnd_in(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint32_t)(hi - lo + 1)); }

struct State {
    int na, ds, chanbits;
    int32_t h[9];   // h[0] = out[j - 1] ... h[na] = out[j - 1 - na] = top
    int16_t a[8];
    int32_t del;
};

// the oracle's coefficients after the one regular step of the row that reaches S
static void oracle_step(const State &S, int16_t (&coefs)[8])
{
    int32_t pc[10], out[10];
    const int na = S.na;
    // out[q] = h[na - q]: sample 0 as it comes, samples 1 .. na first-order
    pc[0] = S.h[na];
    for (int q = 1; q <= na; q++) pc[q] = (int32_t)((uint32_t)S.h[na - q] - (uint32_t)S.h[na - q + 1]);
    pc[na + 1] = S.del;
    for (int i = 0; i < 8; i++) coefs[i] = S.a[i];
    oalac_unpc_block(pc, out, na + 2, coefs, na, (uint32_t)S.chanbits, (uint32_t)S.ds);
    for (int q = 0; q <= na; q++)
        if (out[q] != S.h[na - q]) {
            printf("the warm-up did not reach the history: na %d chanbits %d position %d\n", na, S.chanbits, q);
            exit(1);
        }
}

static long long checked = 0;
static void compare(const char *form, const State &S, const int32_t *got, int slots)
{
    int16_t want[8];
    oracle_step(S, want);
    for (int i = 0; i < slots; i++) {
        const int16_t w = i < S.na ? want[i] : 0;  // a slot that holds no tap keeps the 0 it started with
        if ((int16_t)got[i] != w) {
            printf("%s: na %d denShift %d chanbits %d del %d: coefficient %d is %d, the oracle's %d\n", form, S.na, S.ds, S.chanbits,
                   S.del, i, (int16_t)got[i], w);
            exit(1);
        }
    }
    checked++;
}

static const int32_t kRcMask9 = (1 << 9) - 1;
static int32_t same_sign(int, int32_t sg) { return sg; }

// an 8-slot lane with the lane's own tap count: AnyLane of alac_decode_v1.hip
static void run_any(const State &S)
{
    int32_t a[8], b[8], am[8];
    uint32_t wg[8];
    for (int i = 0; i < 8; i++) {
        am[i] = i < S.na ? -1 : 0;
        wg[i] = i < S.na ? (uint32_t)(S.na - i) : 0u;
        a[i] = i < S.na ? S.a[i] : 0;
        // the window of a dead slot holds real samples
        b[i] = i < S.na ? S.h[S.na] - S.h[i] : rnd_in(-(1 << S.chanbits) + 1, (1 << S.chanbits) - 1);
    }
    lms_adapt_thresholds<8>(a, b, S.del, (1 << S.ds) - 1, S.ds, [&](int i, int32_t sg) { return sg & am[i]; }, [&](int i) { return wg[i]; });
    compare("any", S, a, 8);
}

template <int T>
static void run_wide(const State &S)
{
    int32_t a[T], b[T];
    for (int i = 0; i < T; i++) {
        a[i] = S.a[i];
        b[i] = S.h[T] - S.h[i];
    }
    lms_adapt_thresholds<T>(a, b, S.del, kRcMask9, 9, same_sign, [](int i) { return (uint32_t)(T - i); });
    compare("wide", S, a, T);
}

// T = 8 takes 4-tap chains too: dead upper slots, the lane's own weights on the lower ones
template <int T>
static void run_pair(const State &S)
{
    const bool is4 = S.na == 4;
    const int32_t act = is4 ? 0 : -1;
    uint32_t wg[4];
    for (int i = 0; i < 4; i++) wg[i] = (is4 ? 4u : 8u) - (uint32_t)i;
    int32_t a[T], b[T];
    for (int i = 0; i < T; i++) {
        a[i] = i < S.na ? S.a[i] : 0;
        b[i] = i < S.na ? S.h[S.na] - S.h[i] : rnd_in(-(1 << S.chanbits) + 1, (1 << S.chanbits) - 1);
    }
    lms_adapt_thresholds<T>(
        a, b, S.del, kRcMask9, 9, [&](int i, int32_t sg) { return (T == 8 && i >= 4) ? (sg & act) : sg; },
        [&](int i) { return T == 4 ? (uint32_t)(T - i) : (i < 4 ? wg[i] : (uint32_t)(T - i)); });
    compare("pair", S, a, T);
}

enum { kRandom, kConstant, kAlternating, kSomeEqualTop, kHistories };
static void fill_history(State &S, int kind)
{
    const int32_t lo = -(1 << (S.chanbits - 1)), hi = (1 << (S.chanbits - 1)) - 1;
    const int32_t c = rnd_in(lo, hi);
    for (int i = 0; i <= S.na; i++) {
        switch (kind) {
        case kRandom: S.h[i] = (rnd() & 3) ? rnd_in(lo, hi) : rnd_in(lo < -600 ? -600 : lo, hi > 600 ? 600 : hi); break;  // some near 2^ds
        case kConstant: S.h[i] = c; break;
        case kAlternating: S.h[i] = (i & 1) ? lo : hi; break;
        default: S.h[i] = rnd_in(lo, hi); break;
        }
    }
    if (kind == kSomeEqualTop)  // b_i = 0 on some taps
        for (int i = 0; i < S.na; i++)
            if (rnd() & 1) S.h[i] = S.h[S.na];
}
static void fill_coefs(State &S, int rep)
{
    for (int i = 0; i < 8; i++) {
        switch ((rep + i) % 4) {
        case 0: S.a[i] = (int16_t)rnd_in(-32768, 32767); break;
        case 1: S.a[i] = (int16_t)(32767 - rnd_in(0, 1)); break;  // one step from the int16 wrap
        case 2: S.a[i] = (int16_t)(-32768 + rnd_in(0, 1)); break;
        default: S.a[i] = (int16_t)rnd_in(-300, 300); break;
        }
    }
}

template <typename Run>
static void sweep(int na, int ds, int reps, Run run)
{
    for (int chanbits = 9; chanbits <= 23; chanbits++) {
        const int32_t full = 1 << (chanbits - 1);
        const int32_t small = rnd_in(3, 1 << (chanbits / 2));
        const int32_t dels[] = {0, 1, -1, 2, -2, small, -small, full - 1, -full, rnd_in(-full, full - 1), rnd_in(-40, 40)};
        for (int32_t del : dels)
            for (int kind = 0; kind < kHistories; kind++)
                for (int rep = 0; rep < reps; rep++) {
                    State S;
                    S.na = na;
                    S.ds = ds;
                    S.chanbits = chanbits;
                    S.del = del;
                    fill_history(S, kind);
                    fill_coefs(S, rep);
                    run(S);
                }
    }
}

int main()
{
    for (int na = 1; na <= 8; na++)
        for (int ds = 1; ds <= 15; ds++) sweep(na, ds, 2, run_any);
    const long long nAny = checked;
    sweep(4, 9, 24, run_wide<4>);
    sweep(8, 9, 24, run_wide<8>);
    sweep(4, 9, 24, run_pair<4>);
    sweep(4, 9, 24, run_pair<8>);  // a 4-tap chain in an 8-tap lane
    sweep(8, 9, 24, run_pair<8>);
    printf("%lld states (%lld in the any form), chanBits 9 .. 23; chanBits > 23 is the generic walk's and not covered\n", checked, nAny);
    if (checked < 200000) {
        printf("fewer than 200 000 states\n");
        return 1;
    }
    printf("ok\n");
    return 0;
}
