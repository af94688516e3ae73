// alac_float_rule.hpp — the float32 -> integer rule of alac_hip_encode_float / alac_hip_encode_float_dither as device code:
// the quantization, the saturation, the NaN rule and the TPDF dither.  One spelling for both of its users: the quantize pass
// in front of the encoder (alac_float_in.hip, the float source of pcm_walk, alac_pcm_walk.hpp) and the verifier's store
// sites (alac_hip_verify_float, alac_verify.hpp).  What pins the rule is the numpy restatement of the tests, not a second
// copy here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "alac_kernels.hpp"

namespace alacdev {

// the rule of alac_hip_encode_float: r = rint(x * 2^(DEPTH-1)) (the product is exact), saturated; NaN -> 0.  r is an
// integer, so "r > 2^(DEPTH-1) - 1" is "r >= 2^(DEPTH-1)", a comparison with an exact float even at 32 bits.
template <int DEPTH>
__device__ __forceinline__ int32_t saturate(bool nan, float r, uint32_t &clips)
{
    constexpr float kScale = (float)(1ull << (DEPTH - 1));
    constexpr int32_t kMax = (int32_t)((1ull << (DEPTH - 1)) - 1);
    const bool hi = r >= kScale;
    clips += (nan || hi || r < -kScale) ? 1u : 0u;
    // fmaxf(NaN, y) = y, so the conversion only ever sees a value in [-2^(DEPTH-1), 2^(DEPTH-1))
    const int32_t s = (int32_t)fmaxf(r, -kScale);
    return nan ? 0 : (hi ? kMax : s);
}

template <int DEPTH>
__device__ __forceinline__ int32_t quantize(float x, uint32_t &clips)
{
    return saturate<DEPTH>(x != x, rintf(x * (float)(1ull << (DEPTH - 1))), clips);
}

// the rule of alac_hip_encode_float_dither: v = x * 2^(DEPTH-1) + d rounded once (the product is exact, so the fused form
// and multiply-then-add agree), r = rint(v), then as above.  d = 0 gives quantize(x).
template <int DEPTH>
__device__ __forceinline__ int32_t quantize_dithered(float x, float d, uint32_t &clips)
{
    return saturate<DEPTH>(x != x, rintf(fmaf(x, (float)(1ull << (DEPTH - 1)), d)), clips);
}

// ---- TPDF dither: Philox4x32-10 (Salmon et al., Random123), a pure function of (seed, channel, frame index) ----
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

// counter (T & 0xffffffff, T >> 32, c, 0): two 32 x 32 -> 64-bit products per round, both halves of each used
__device__ __forceinline__ void philox(uint64_t T, uint32_t c, const FloatDitherArgs &d, uint32_t (&w)[4])
{
    uint32_t c0 = (uint32_t)T, c1 = (uint32_t)(T >> 32), c2 = c, c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ d.roundKey[r][0], n2 = (uint32_t)(p0 >> 32) ^ c3 ^ d.roundKey[r][1];
        c0 = n0, c1 = (uint32_t)p1, c2 = n2, c3 = (uint32_t)p0;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// the integer of the dither rule, k = (wa >> 8) - (wb >> 8): |k| < 2^24, triangular.  The integer rule of
// alac_hip_pcm_requantize (alac_pcm_in.hip) adds it to a fixed-point accumulator as it is
__device__ __forceinline__ int32_t tpdf_k(uint32_t wa, uint32_t wb)
{
    return (int32_t)(wa >> 8) - (int32_t)(wb >> 8);
}

// k * 2^-24: |k| < 2^24, so the conversion and the scaling are exact
__device__ __forceinline__ float tpdf(uint32_t wa, uint32_t wb)
{
    return (float)tpdf_k(wa, wb) * 0x1p-24f;
}

// the k of channel c at stream frames t0 .. t0 + 3.  One Philox call serves frames 2T and 2T + 1: two calls when t0 is
// even (every word used), three when it is odd (an odd packet origin; the same for a whole wave, so no divergence).
__device__ __forceinline__ void dither4_k(uint64_t t0, uint32_t c, const FloatDitherArgs &d, int32_t (&k)[4])
{
    const uint64_t T = t0 >> 1;
    uint32_t u[4], v[4];
    philox(T, c, d, u);
    philox(T + 1, c, d, v);
    if ((t0 & 1) == 0) {
        k[0] = tpdf_k(u[0], u[1]), k[1] = tpdf_k(u[2], u[3]), k[2] = tpdf_k(v[0], v[1]), k[3] = tpdf_k(v[2], v[3]);
    } else {
        uint32_t w[4];
        philox(T + 2, c, d, w);
        k[0] = tpdf_k(u[2], u[3]), k[1] = tpdf_k(v[0], v[1]), k[2] = tpdf_k(v[2], v[3]), k[3] = tpdf_k(w[0], w[1]);
    }
}

// the same as the float d = k * 2^-24 of the float rule
__device__ __forceinline__ void dither4(uint64_t t0, uint32_t c, const FloatDitherArgs &d, float (&z)[4])
{
    int32_t k[4];
    dither4_k(t0, c, d, k);
#pragma unroll
    for (int j = 0; j < 4; j++) z[j] = (float)k[j] * 0x1p-24f;
}

}  // namespace alacdev
