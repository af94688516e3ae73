// alac_lms.hpp — the adaptive predictor (pc_block, codec/dp_enc.c:77-388) for gfx950, wave64.
//
// Lane mapping: a chain (one channel of one packet) owns LPC adjacent lanes, each lane holds 4 taps
// (coefficients and the matching 4-sample history window in registers):
//   LPC = 2   8-tap rows: lane h = 0 holds taps 0..3, lane h = 1 taps 4..7; the tap sum of a step is the
//             in-lane 4-term multiply-add chain plus ONE cross-lane add (DPP quad_perm xor 1)
//   LPC = 1   4-tap rows: the whole chain lives in one lane, no cross-lane traffic at all
// so a wave walks 32 (LPC 2) or 64 (LPC 1) chains at once.  With 10 000 stereo packets that is 625 waves,
// i.e. at most one wave per SIMD on 1024 SIMDs: the cost of a step is this wave's own instruction count,
// which is why the taps are folded into the lanes instead of being spread over 8 lanes each.
//
// The early-exit update walk of the reference ("for k = na-1 .. 0 while del0 keeps its sign",
// dp_enc.c:143-188) is evaluated without the walk: with t_i = |b_i| >> 9 (del > 0) resp.
// (|b_i| + 511) >> 9 (del < 0) [= -((-|b_i|) >> 9)], tap k is touched iff
// |del| > S_k := sum_{i > k} (na - i) * t_i, because the partial sums only grow.
#pragma once

#include <stdint.h>
#if defined(__HIPCC__)
#include "alac_dev.hpp"
#define ALAC_RULE_FN __device__ __forceinline__
#else  // a host compiler sees lms_adapt_thresholds alone (tests/cpp/lms_rule.cpp): its qualifiers and primitives in plain C++
#include <algorithm>
#define ALAC_RULE_FN inline
#endif

namespace alacdev {

#if defined(__HIPCC__)
constexpr int kDppXor1 = 0xB1;  // quad_perm:[1,0,3,2]: partner lane of a 2-lane chain

__device__ __forceinline__ int32_t dpp_xor1(int32_t src)
{
    return __builtin_amdgcn_update_dpp(0, src, kDppXor1, 0xf, 0xf, true);
}

__device__ __forceinline__ int32_t med3_i32(int32_t x, int32_t lo, int32_t hi)
{
    int32_t r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(lo), "v"(hi));
    return r;
}

// sign(x) as clamp(x, -1, 1) in one v_med3_i32 with inline constants
__device__ __forceinline__ int32_t sign3(int32_t x)
{
    int32_t r;
    asm("v_med3_i32 %0, %1, -1, 1" : "=v"(r) : "v"(x));
    return r;
}
#else
using std::max;
inline int32_t sign3(int32_t x) { return x > 0 ? 1 : (x < 0 ? -1 : 0); }
// v_mul_i32_i24 / v_mul_u32_u24: the low 24 bits of each operand, the low 32 bits of the product
inline int32_t __mul24(int32_t x, int32_t y) { return (int32_t)(uint32_t)((int64_t)((int32_t)((uint32_t)x << 8) >> 8) * ((int32_t)((uint32_t)y << 8) >> 8)); }
inline uint32_t __umul24(uint32_t x, uint32_t y) { return (uint32_t)((uint64_t)(x & 0xffffffu) * (y & 0xffffffu)); }
#endif

// ---- the coefficient update of a step, the walk in threshold form (top of this file): the one spelling of the decoder's
// one-lane steps (lms_step_dec_wide / _any / _pair, alac_decode_v1.hip).  b[i] = top - in[j - 1 - k] for the tap k of slot i,
// a[i] its coefficient (an int16 value in an int32); sign(i, sg): sg, or 0 for a slot that holds no tap; weight(i): na - k.
// No term may wrap: |b| < 2^23 (chanBits <= 23).  Two steps keep their own copy: lms4_step_dec below was joined (its carry
// one more callable) and taken out again — k_dec_fused_wg's step loop then split two v_add_u32_dpp into v_mov_b32_dpp +
// v_add_u32 and the fused launch measured 0.3 % slower at 10 000 packets; joining the encoder's lms_step was not tried.
template <int T, typename Sign, typename Weight>
ALAC_RULE_FN void lms_adapt_thresholds(int32_t (&a)[T], const int32_t (&b)[T], int32_t del, int32_t rcMask, int32_t ds, Sign sign,
                                       Weight weight)
{
    // t_i = (|b_i| + rc) >> ds with rc = 2^ds - 1 for del < 0 (the arithmetic shift of a negative product rounds away from
    // zero, dp_enc.c:176), S_{i-1} = t_i * weight_i + S_i, tap i is touched iff |del| > S_i
    const int32_t nd = -del;
    const int32_t adel = max(del, nd);
    const int32_t nsg = sign3(nd);  // -sign(del): what a touched tap adds per sign(b)
    const int32_t rc = (del >> 31) & rcMask;
    int32_t sb[T];
    uint32_t t[T];
#pragma unroll
    for (int i = 0; i < T; i++) {
        sb[i] = sign(i, sign3(b[i]));
        t[i] = (uint32_t)(__mul24(sb[i], b[i]) + rc) >> ds;  // |b| = sign(b) * b
    }
    int32_t S[T];  // in-lane part of S_k, from the top tap down
    S[T - 1] = 0;
#pragma unroll
    for (int i = T - 1; i > 0; i--) S[i - 1] = (int32_t)__umul24(t[i], weight(i)) + S[i];
#pragma unroll
    for (int i = 0; i < T; i++) a[i] = __mul24(adel > S[i] ? nsg : 0, sb[i]) + a[i];
}

#if defined(__HIPCC__)
// ---- lane mappings --------------------------------------------------------------------------------------
// A chain owns L adjacent lanes (L = 1, 2 or 4, inside one DPP quad), each lane T taps: <T, L> covers T * L >= na taps.
//   <4, 1>  4-tap rows, one lane per chain (64 chains per wave)
//   <4, 2>  8-tap rows, two lanes per chain (32 chains per wave): the shape of the searches at every batch size and
//           of 4- and 8-tap rows in the final pass of mid-size batches
//   <8, 1>  8-tap rows in ONE lane (64 chains per wave): fewest instructions per chain step (throughput regime)
//   <2, 2>  4-tap rows over two lanes, <2, 4> 8-tap rows over four lanes: fewest instructions per WAVE step (the
//           latency regime of the final pass, where the chains of one class fit one wave per SIMD)
// Tap k = T * h + i lives in lane h = lane % L, slot i.

constexpr int kDppXor2 = 0x4E;  // quad_perm:[2,3,0,1]
constexpr int kDppShl1 = 0xF9;  // quad_perm:[1,2,3,3]: lane q reads lane q + 1 of its quad
constexpr int kDppShl2 = 0xFE;  // quad_perm:[2,3,3,3]: lane q reads lane q + 2 of its quad

template <int CTRL>
__device__ __forceinline__ int32_t dpp_quad(int32_t src)
{
    return __builtin_amdgcn_update_dpp(0, src, CTRL, 0xf, 0xf, true);
}

// per-lane constants of a chain
template <int T>
struct LmsLaneT {
    int32_t h;         // which group of T taps this lane holds (always 0 for L = 1)
    int32_t na;        // taps of the chain (4 or 8)
    int32_t wg[T];     // update weights na - (T h + i), 0 for taps >= na
    int32_t act[T];    // ~0 for taps < na (only consulted where a LANE can hold both kinds: T = 8 with a 4-tap row)
    int32_t c255;      // 255 on the lane holding tap 0: folds "denhalf - sum" into the product chain
    int32_t carry1;    // ~0 where lane h + 1 belongs to the chain: it takes that lane's threshold total
    int32_t carry2;    // ~0 where lane h + 2 belongs to the chain (L = 4)
    int32_t jlo, jhi;  // coefficients adapt for jlo <= j < jhi (jlo = na + 1, jhi = pc_block's num)
};

template <int T, int L>
__device__ __forceinline__ LmsLaneT<T> make_lane(int lane, int na, int num)
{
    LmsLaneT<T> R;
    R.h = L == 1 ? 0 : (lane & (L - 1));
    R.na = na;
#pragma unroll
    for (int i = 0; i < T; i++) {
        const int kk = T * R.h + i;
        R.wg[i] = kk < na ? na - kk : 0;
        R.act[i] = kk < na ? -1 : 0;
    }
    R.c255 = R.h == 0 ? 255 : 0;
    R.carry1 = (R.h + 1 < L) ? -1 : 0;
    R.carry2 = (R.h + 2 < L) ? -1 : 0;
    R.jlo = na + 1;
    R.jhi = num;
    return R;
}

// One predictor step of every chain of the wave.
//   a[i]  coefficient of tap T h + i (int16 value carried in an int32; the wrap is applied where it is read)
//   w[i]  in[j-1-(T h + i)]   (lanes holding no active tap are fed zeros: b = 0, nothing happens)
//   tp    in[j-1-na] ("top"),  cu = in[j]
// Returns the residual.  sum1 = (denhalf - sum) >> 9 and del = in[j] - top - sum1 (dp_enc.c:136-139)
// are folded into del = (in[j] - top) + ((sum + 255) >> 9): -floor((256 - s)/512) == floor((s + 255)/512).
// DEAD: the lane may hold taps beyond its row's own count (a 4-tap row in an 8-tap lane: k_class_final<.., 8>); kernels whose
// rows always fill the lane (the in-lane searches) pass false and save the mask per tap
template <int T, int L, bool MASKED, bool DEAD = (T > 4)>
__device__ __forceinline__ int32_t lms_step(int32_t (&a)[T], const int32_t (&w)[T], int32_t tp, int32_t cu,
                                            int32_t liveMask, const LmsLaneT<T> &R, uint32_t chanbits)
{
    // The step is written for the fewest instructions: the residual first, then ONE set of thresholds with the rounding
    // its sign selects (an earlier version evaluated both roundings ahead of del: 73 instructions per step against 50).
    // Measured rule for a wave that has a SIMD to itself (DESIGN 4.0 "step schedule", profiles/step_schedule/): it pays about
    // 6 cycles for every instruction it issues, a hazard pad included, whether or not the instruction reads what its
    // neighbour wrote.  lms_step_lone below runs the same arithmetic in a fixed order with 2.5 instead of 14 directly
    // dependent neighbours and 0.5 instead of 3.5 pads a step, the same instructions otherwise; the three launches gained
    // 3.3 / 2.3 / 1.4 % (8 to 12 cycles a step): the worth of the pads.  The 2.6 cycles a dependent pair that the
    // microbenchmark's two figures (7.4 dependent, 4.8 independent) suggest do not show in this loop.
    int32_t b[T];
#pragma unroll
    for (int i = 0; i < T; i++) b[i] = tp - w[i];
    const int32_t p = cu - tp;
    int32_t s = R.c255;
#pragma unroll
    for (int i = 0; i < T; i++) s = __mul24((int32_t)(int16_t)a[i], b[i]) + s;
    if constexpr (L >= 2) s += dpp_xor1(s);
    if constexpr (L == 4) s += dpp_quad<kDppXor2>(s);
    const int32_t del = __builtin_amdgcn_sbfe(p + (s >> kDenShift), 0, chanbits);

    // coefficient walk: t_i = (|b_i| + rc) >> 9 with rc = 511 for del < 0 (the arithmetic shift of a negative
    // product rounds away from zero, dp_enc.c:176), tap k is touched iff |del| > S_k
    const int32_t nd = -del;
    const int32_t adel = max(del, nd);
    int32_t nsg = sign3(nd);                // -sign(del): what a touched tap adds per sign(b)
    if constexpr (MASKED) nsg &= liveMask;  // steps outside [jlo, jhi) leave the coefficients alone
    const int32_t rc = (del >> 31) & ((1 << kDenShift) - 1);
    int32_t sb[T];
    uint32_t t[T];
#pragma unroll
    for (int i = 0; i < T; i++) {
        sb[i] = sign3(b[i]);
        // A lane that holds no active tap at all is fed zeros (b = 0: nothing happens).  With 8 taps in one lane a 4-tap
        // row (the narrower channel of a packet of the 8-tap class) has dead taps BESIDE live ones: their window holds
        // real samples, so their sign is forced to 0 — then t = 0, the coefficient stays 0 and the tap sum ignores it.
        if constexpr (DEAD) sb[i] &= R.act[i];
        t[i] = (uint32_t)(__mul24(sb[i], b[i]) + rc) >> kDenShift;  // |b| = sign(b) * b
    }
    int32_t S[T];  // in-lane part of S_k, from the top tap down
    S[T - 1] = 0;
#pragma unroll
    for (int i = T - 1; i > 0; i--) S[i - 1] = (int32_t)__umul24(t[i], (uint32_t)R.wg[i]) + S[i];
    int32_t adj = adel;
    if constexpr (L >= 2) {
        // the lower taps also count everything the lanes above hold: |del| > S + c  <=>  |del| - c > S
        const int32_t tot = (int32_t)__umul24(t[0], (uint32_t)R.wg[0]) + S[0];
        if constexpr (L == 2) {
            adj = adel - (dpp_xor1(tot) & R.carry1);
        } else {
            const int32_t up1 = dpp_quad<kDppShl1>(tot) & R.carry1;          // total of lane h + 1
            const int32_t pair = tot + up1;                                   // lanes h, h + 1
            adj = adel - up1 - (dpp_quad<kDppShl2>(pair) & R.carry2);         // + lanes h + 2, h + 3
        }
    }
#pragma unroll
    for (int i = 0; i < T; i++) a[i] = __mul24(adj > S[i] ? nsg : 0, sb[i]) + a[i];
    return del;
}

// ---- the step of a wave that owns its SIMD (LONE), <4, 1> and <4, 2> ---------------------------------------------
// The same arithmetic as lms_step in a fixed instruction order (what it bought: the comment in lms_step).  The order keeps
// the instructions of the serial chain (tap sum -> del -> thresholds -> selects -> coefficients -> next tap sum) apart:
// the step's own side values (nd, adel, nsg) and the caller's fillers sit between them — fill.sub(n): n of the plain
// subtractions that form a LATER step's b = tp - w and cu - tp, fill.sgn(): one sign3(b) of a later step.  The four compares
// come first and the four selects after them (no pad between a compare and its select), and two subtractions stand ahead
// of each DPP exchange.  The operands b, sign3(b) and p = cu - tp come prepared; the products of the NEXT step (bn = its
// b) are formed as the coefficients appear and carried to it in C.
struct LoneCarry {
    int32_t s1, m1, m0;  // m3 + m2 + c255 and the products of taps 1, 0 of the step to come
};

// ALAC_PIN(x): x is complete here and nothing crosses — the empty volatile asm keeps the instruction that forms x ahead of
// this point, the barrier keeps the scheduler from moving anything over it.  The asm only READS x: one that also wrote it
// would hide the instruction that did from the hazard checks, which then pad whatever reads x next.
#define ALAC_PIN(x)                          \
    do {                                     \
        asm volatile("" : : "v"(x));         \
        __builtin_amdgcn_sched_barrier(0);   \
    } while (0)
// ALAC_ARM(x): nothing that reads x is placed ahead of this point (the asm writes x in place: keep one instruction between
// this and the reader)
#define ALAC_ARM(x) asm volatile("" : "+v"(x))

// sign3 as a filler: volatile, so that it stays in the gap it was written into (the hazard checks count an asm statement
// as no instruction at all: this one fills a gap of the chain but never one of the two slots ahead of a DPP exchange)
__device__ __forceinline__ int32_t sign3_pinned(int32_t x)
{
    int32_t r;
    asm volatile("v_med3_i32 %0, %1, -1, 1" : "=v"(r) : "v"(x));
    __builtin_amdgcn_sched_barrier(0);
    return r;
}

__device__ __forceinline__ void lone_products(LoneCarry &C, const int32_t (&a)[4], const int32_t (&bn)[4], const LmsLaneT<4> &R)
{
    C.s1 = __mul24((int32_t)(int16_t)a[3], bn[3]) + __mul24((int32_t)(int16_t)a[2], bn[2]) + R.c255;
    C.m1 = __mul24((int32_t)(int16_t)a[1], bn[1]);
    C.m0 = __mul24((int32_t)(int16_t)a[0], bn[0]);
}

// fill.sub(): one (two for L = 1) of the plain subtractions b = tp - w / p = cu - tp, fill.sgn(): one sign3(b)
template <int L, bool MASKED, class Fill>
__device__ __forceinline__ int32_t lms_step_lone(int32_t (&a)[4], LoneCarry &C, const int32_t (&b)[4], const int32_t (&sb)[4],
                                                 int32_t p, const int32_t (&bn)[4], int32_t liveMask, const LmsLaneT<4> &R,
                                                 uint32_t chanbits, Fill &&fill)
{
    static_assert(L == 1 || L == 2, "the lone-wave mappings");
    constexpr int32_t kRc = (1 << kDenShift) - 1;
    int32_t s = C.s1 + C.m1 + C.m0;
    ALAC_PIN(s);
    if constexpr (L == 2) {
        fill.sub(2);
        s += dpp_xor1(s);
        ALAC_PIN(s);
    }
    fill.sgn();
    s >>= kDenShift;
    ALAC_PIN(s);
    fill.sgn();
    s += p;
    ALAC_PIN(s);
    fill.sgn();
    int32_t del = __builtin_amdgcn_sbfe(s, 0, chanbits);
    ALAC_PIN(del);
    fill.sgn();
    int32_t nd = -del;
    ALAC_PIN(nd);
    int32_t rc = del >> 31;
    ALAC_PIN(rc);
    int32_t adel = max(del, nd);
    ALAC_PIN(adel);
    rc &= kRc;
    ALAC_PIN(rc);
    int32_t nsg = sign3_pinned(nd);  // -sign(del): what a touched tap adds per sign(b)
    if constexpr (MASKED) {
        nsg &= liveMask;  // steps outside [jlo, jhi) leave the coefficients alone
        ALAC_PIN(nsg);
    }
    // thresholds from the top tap down (lms_adapt_thresholds): t_i = (|b_i| + rc) >> 9, S_{i-1} = t_i w_i + S_i
    int32_t u3 = __mul24(sb[3], b[3]) + rc;
    ALAC_PIN(u3);
    int32_t u2 = __mul24(sb[2], b[2]) + rc;
    ALAC_PIN(u2);
    int32_t t3 = (int32_t)((uint32_t)u3 >> kDenShift);
    ALAC_PIN(t3);
    int32_t u1 = __mul24(sb[1], b[1]) + rc;
    ALAC_PIN(u1);
    int32_t t2 = (int32_t)((uint32_t)u2 >> kDenShift);
    ALAC_PIN(t2);
    int32_t S2 = (int32_t)__umul24((uint32_t)t3, (uint32_t)R.wg[3]);
    ALAC_PIN(S2);
    int32_t u0 = 0;
    if constexpr (L == 2) {
        u0 = __mul24(sb[0], b[0]) + rc;
        ALAC_PIN(u0);
    }
    int32_t t1 = (int32_t)((uint32_t)u1 >> kDenShift);
    ALAC_PIN(t1);
    int32_t S1 = (int32_t)__umul24((uint32_t)t2, (uint32_t)R.wg[2]) + S2;
    ALAC_PIN(S1);
    int32_t S0, adj;
    if constexpr (L == 2) {
        // the lower taps also count everything the lane above holds: |del| > S + c  <=>  |del| - c > S
        int32_t t0 = (int32_t)((uint32_t)u0 >> kDenShift);
        ALAC_PIN(t0);
        S0 = (int32_t)__umul24((uint32_t)t1, (uint32_t)R.wg[1]) + S1;
        ALAC_PIN(S0);
        fill.sub(1);
        int32_t tot = (int32_t)__umul24((uint32_t)t0, (uint32_t)R.wg[0]) + S0;
        ALAC_PIN(tot);
        fill.sub(2);
        int32_t up = dpp_xor1(tot) & R.carry1;
        ALAC_PIN(up);
        adj = adel - up;
        ALAC_PIN(adj);
    } else {
        fill.sub(2);
        S0 = (int32_t)__umul24((uint32_t)t1, (uint32_t)R.wg[1]) + S1;
        ALAC_PIN(S0);
        fill.sub(2);
        adj = adel;
    }
    // four compares into four scalar pairs, then the selects: no select waits for its compare
    const bool c3 = adj > 0;
    __builtin_amdgcn_sched_barrier(0);
    const bool c2 = adj > S2;
    __builtin_amdgcn_sched_barrier(0);
    const bool c1 = adj > S1;
    __builtin_amdgcn_sched_barrier(0);
    const bool c0 = adj > S0;
    __builtin_amdgcn_sched_barrier(0);
    // (one lane: adj is |del| itself, and nsg is already 0 where that is 0)
    int32_t g3 = L == 1 ? nsg : (c3 ? nsg : 0);
    if constexpr (L == 2) ALAC_PIN(g3);
    int32_t g2 = c2 ? nsg : 0;
    ALAC_PIN(g2);
    a[3] = __mul24(g3, sb[3]) + a[3];
    ALAC_PIN(a[3]);
    int32_t g1 = c1 ? nsg : 0;
    ALAC_PIN(g1);
    a[2] = __mul24(g2, sb[2]) + a[2];
    ALAC_PIN(a[2]);
    int32_t n3 = __mul24((int32_t)(int16_t)a[3], bn[3]);
    ALAC_PIN(n3);
    int32_t g0 = c0 ? nsg : 0;
    ALAC_PIN(g0);
    a[1] = __mul24(g1, sb[1]) + a[1];
    ALAC_PIN(a[1]);
    int32_t n2 = __mul24((int32_t)(int16_t)a[2], bn[2]);
    ALAC_PIN(n2);
    a[0] = __mul24(g0, sb[0]) + a[0];
    ALAC_PIN(a[0]);
    C.m1 = __mul24((int32_t)(int16_t)a[1], bn[1]);
    ALAC_PIN(C.m1);
    C.s1 = n3 + n2 + R.c255;
    ALAC_PIN(C.s1);
    C.m0 = __mul24((int32_t)(int16_t)a[0], bn[0]);
    ALAC_PIN(C.m0);
    if constexpr (L == 1) fill.sub(1);
    return del;
}

// the two shapes every kernel used before the lane mappings became a template parameter
using LmsLane = LmsLaneT<4>;
template <int LPC, bool MASKED>
__device__ __forceinline__ int32_t lms4_step(int32_t (&a)[4], const int32_t (&w)[4], int32_t tp, int32_t cu,
                                             int32_t liveMask, const LmsLane &R, uint32_t chanbits)
{
    return lms_step<4, LPC, MASKED>(a, w, tp, cu, liveMask, R, chanbits);
}

// ---- decode direction (unpc_block, codec/dp_dec.c:55-381) with the same lane mapping ----
// The residual `del` is an INPUT here, so the coefficient update (same thresholds, same signs as pc_block) is off
// the dependent chain altogether; what is serial is out[j-1] -> b_0 -> tap sum -> out[j].  The history windows
// hold the chain's own outputs: lane h = 0 keeps out[j-1..j-4], lane h = 1 out[j-5..j-8]; the sample leaving
// lane 0's window enters lane 1's, and the one leaving the window of the last active tap is the next "top"
// (one DPP exchange per step for both).
struct LmsDecLane {
    int32_t h;
    int32_t wg[4];
    int32_t c255, carryMask;
    int32_t topMine;   // -1 on the lane whose dropped sample becomes the next top (h = 1 for 8 taps, h = 0 for 4)
    int32_t takeOut;   // -1 on h = 0: the new output enters this lane's window
    int32_t feed;      // 0 on a lane that holds no active tap (h = 1 of a 4-tap chain): it is fed zeros, so its
                       // b, its signs and therefore its coefficients stay 0
};

__device__ __forceinline__ LmsDecLane make_dec_lane(int lane, int na)
{
    LmsDecLane L;
    L.h = lane & 1;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int kk = 4 * L.h + i;
        L.wg[i] = kk < na ? na - kk : 0;
    }
    L.c255 = L.h == 0 ? 255 : 0;
    L.carryMask = L.h == 0 ? -1 : 0;
    L.topMine = (L.h == (na == 8 ? 1 : 0)) ? -1 : 0;
    L.takeOut = L.h == 0 ? -1 : 0;
    L.feed = (L.h == 0 || na == 8) ? -1 : 0;
    return L;
}

// one unpc step: returns out[j]; updates a[], the window w[] and tp (the "top" of the NEXT step)
__device__ __forceinline__ int32_t lms4_step_dec(int32_t (&a)[4], int32_t (&w)[4], int32_t &tp, int32_t del,
                                                 const LmsDecLane &L, uint32_t chanbits)
{
    int32_t b[4];
#pragma unroll
    for (int i = 0; i < 4; i++) b[i] = tp - w[i];
    // out[j] = sext(del + top + ((denhalf - sum) >> 9)), -((256 - s) >> 9) == (s + 255) >> 9
    int32_t s = L.c255;
#pragma unroll
    for (int i = 0; i < 4; i++) s = __mul24((int32_t)(int16_t)a[i], b[i]) + s;
    s += dpp_xor1(s);
    const int32_t out = __builtin_amdgcn_sbfe(del + tp - (s >> kDenShift), 0, chanbits);

    // coefficient update, driven by del (dp_dec.c:143-188 == the encoder's walk, same form as lms4_step)
    const int32_t nd = -del;
    const int32_t adel = max(del, nd);
    const int32_t nsg = sign3(nd);
    const int32_t rc = (del >> 31) & ((1 << kDenShift) - 1);
    int32_t sb[4];
    uint32_t t[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        sb[i] = sign3(b[i]);
        t[i] = (uint32_t)(__mul24(sb[i], b[i]) + rc) >> kDenShift;
    }
    int32_t S[4];
    S[3] = 0;
#pragma unroll
    for (int i = 3; i > 0; i--) S[i - 1] = (int32_t)__umul24(t[i], (uint32_t)L.wg[i]) + S[i];
    const int32_t tot = (int32_t)__umul24(t[0], (uint32_t)L.wg[0]) + S[0];
    const int32_t adj = adel - (dpp_xor1(tot) & L.carryMask);
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = __mul24(adj > S[i] ? nsg : 0, sb[i]) + a[i];
    // windows: lane 0's oldest sample moves to lane 1, the oldest sample of the last active tap is the next top
    const int32_t x = dpp_xor1(w[3]) & L.feed;
    tp = L.topMine ? w[3] : x;
    w[3] = w[2];
    w[2] = w[1];
    w[1] = w[0];
    w[0] = L.takeOut ? out : x;
    return out;
}

#endif  // __HIPCC__

}  // namespace alacdev

#undef ALAC_RULE_FN
