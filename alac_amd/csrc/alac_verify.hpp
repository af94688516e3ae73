// alac_verify.hpp — what the decoders' PCM store sites do: store (alac_hip_decode), verify (alac_hip_verify), float
// (alac_hip_decode_float), verify against a float32 source (alac_hip_verify_float) or store into integer containers of the
// caller's layout (alac_hip_decode_int).
//
// Every kernel that writes PCM is instantiated once per PcmMode.  The integer sites write through PCM_PUT(MODE, A, ptr, value).
// With kPcmStore that is the plain store `*ptr = value` it always was, through the site's own pointer type (its alignment
// included: a template would deduce the canonical vector type and assume 16-byte alignment), so the instantiation the decode
// entry point launches is unchanged.
// With kPcmVerify, DecodeArgs::pcmOut is the caller's expected PCM in the layout alac_hip_decode writes: the site loads
// the same bytes through the same pointer (a load as wide as the store), and where they differ lowers firstMismatch[packet]
// to the frame of the first differing byte.  Nothing is stored, so a verify pass reads the expected PCM where a decode
// pass writes the decoded PCM.
// With kPcmFloat, DecodeArgs::pcmOut is planar float32: sample j of channel c of packet p at
// pcm_float_row(A, c, p)[j], the value pcm_float<DEPTH>(sample).  Several sites hand PCM_PUT packed words (two 16-bit
// samples, four 3-byte fields in three words, single bytes), which a float store cannot be made from, so every site has a
// sample branch of its own in front of the packing, on the sample values it holds (the branch of every mode that works by
// sample, pcm_by_sample); PCM_PUT refuses to compile in those modes, so a site without one cannot slip through.  The branch
// calls pcm_sample_put (one sample) or pcm_sample_run (four or more consecutive frames of a channel, which float mode writes
// with 16-byte stores: pcm_float_run).
// With kPcmVerifyFloat, DecodeArgs::pcmOut is the caller's float32 SOURCE, only ever read, and the mode's own words travel
// in the PcmModeArgs block that the PCM-writing kernels take as their last argument (alac_kernels.hpp).  The mode lives in the
// sample branches: through pcm_sample_put / pcm_sample_run a site loads the source float of the sample it would have stored,
// computes the integer the float encode path stages for it (alac_float_rule.hpp: the one spelling of the rule) and compares
// that with the decoded sample, sign-extended at the stream's depth.  Every site passes the frame limit pcm_frames gave it —
// min(decoded, expected, frameSize) — and no address is formed for a frame at or behind it, whatever the packet claims to
// hold.  Nothing is stored.
// With kPcmInt, DecodeArgs::pcmOut is the caller's integer destination and the layout travels in the same trailing block.  It
// lives in the sample branches too, behind the same two helpers: the sample a site holds, sign-extended at the stream's depth
// and shifted, goes into its container — 2, 3 or 4 bytes, a packed 3-byte container as exactly its three bytes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "alac_kernels.hpp"
#include "alac_float_rule.hpp"

namespace alacdev {

enum PcmMode : int { kPcmStore = 0, kPcmVerify = 1, kPcmFloat = 2, kPcmVerifyFloat = 3, kPcmInt = 4 };
// the modes whose sites work on sample values per channel (their sample branches)
constexpr bool pcm_by_sample(PcmMode m) { return m == kPcmFloat || m == kPcmVerifyFloat || m == kPcmInt; }

// float mode: a decoded sample as alac_hip_decode stores it (its low DEPTH bits, sign-extended — a 16-bit sample that a damaged
// packet let grow past 16 bits wraps as the int16 store wraps it) times 2^-(DEPTH - 1).  The conversion rounds to nearest
// even (v_cvt_f32_i32), the scaling by a power of two is exact: exact for 16 / 20 / 24 bits; 32-bit samples from
// 2^31 - 64 up round to 1.0
template <int DEPTH>
__device__ __forceinline__ float pcm_float(int32_t x)
{
    constexpr float kScale = 1.0f / (float)(1ull << (DEPTH - 1));
    const int32_t s = DEPTH == 32 ? x : (int32_t)((uint32_t)x << (32 - DEPTH)) >> (32 - DEPTH);
    return (float)s * kScale;
}

// float mode: the row of channel c of packet p
__device__ __forceinline__ float *pcm_float_row(const DecodeArgs &A, uint32_t c, uint32_t p)
{
    return (float *)A.pcmOut + c * A.channelStride + (uint64_t)p * A.frameSize;
}

// float mode: NF consecutive frames f0 .. f0 + NF - 1 of one channel, those in front of n; groups of four as one 16-byte store
// (4-byte alignment is all the output promises: the address is a float index of any frame size)
template <int DEPTH, int NF>
__device__ __forceinline__ void pcm_float_run(float *row, uint32_t f0, uint32_t n, const int32_t (&x)[NF])
{
    typedef float F4 __attribute__((ext_vector_type(4), aligned(4)));
    static_assert(NF % 4 == 0, "whole groups of four frames");
#pragma unroll
    for (int q = 0; q < NF / 4; q++) {
        const uint32_t f = f0 + 4 * q;
        if (f + 4 <= n) {
            const F4 t = {pcm_float<DEPTH>(x[4 * q]), pcm_float<DEPTH>(x[4 * q + 1]), pcm_float<DEPTH>(x[4 * q + 2]),
                          pcm_float<DEPTH>(x[4 * q + 3])};
            *(F4 *)(row + f) = t;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (f + e < n) row[f + e] = pcm_float<DEPTH>(x[4 * q + e]);
        }
    }
}

// ---- verify-float mode (alac_hip_verify_float) ----

// how many frames of packet p a site may touch when the decoder produced n: n itself, except in verify-float mode, where a
// frame at or behind min(expected[p], frameSize) is never loaded from the source (a damaged or foreign packet may decode
// more frames than the caller's tensor holds).  k_verify_finish settles the frames behind the shorter count.
template <PcmMode MODE>
__device__ __forceinline__ uint32_t pcm_frames(const DecodeArgs &A, const PcmModeArgs &F, uint32_t p, uint32_t n)
{
    if constexpr (MODE != kPcmVerifyFloat) return n;
    const uint32_t e = F.numSamplesExpected ? F.numSamplesExpected[p] : A.frameSize;
    return min(n, min(e, A.frameSize));
}
// a bound a site derived from n (n rounded down to whole groups), under the limit pcm_frames gave
template <PcmMode MODE>
__device__ __forceinline__ uint32_t pcm_clamp(uint32_t bound, uint32_t lim)
{
    if constexpr (MODE != kPcmVerifyFloat) return bound;
    return min(bound, lim);
}

// the same "plain load of the current minimum, then atomicMin" as pcm_mismatch; the site knows packet and frame
__device__ __forceinline__ void vf_mismatch(const PcmModeArgs &F, uint32_t p, uint32_t frame)
{
    uint32_t *slot = F.firstMismatch + p;
    if (frame < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, frame);
}
// source float of frame j (of the batch: p * frameSize + i) of channel c
__device__ __forceinline__ const float *vf_source(const DecodeArgs &A, const PcmModeArgs &F, uint32_t c, uint64_t j)
{
    return (const float *)A.pcmOut + c * F.channelStride + j * F.frameStride;
}
// stream frame index of frame 0 of packet p
__device__ __forceinline__ uint64_t vf_origin(const DecodeArgs &A, const PcmModeArgs &F, uint32_t p)
{
    return F.dz.origin ? F.dz.origin[p] : (uint64_t)p * A.frameSize;
}
// does decoded sample `got` differ from what the float encode path stages for source x with dither d (0: no dither —
// quantize_dithered(x, 0) is quantize(x))
template <int DEPTH>
__device__ __forceinline__ bool vf_differs(float x, float d, int32_t got)
{
    uint32_t clips = 0;
    const int32_t s = DEPTH == 32 ? got : (int32_t)((uint32_t)got << (32 - DEPTH)) >> (32 - DEPTH);
    return quantize_dithered<DEPTH>(x, d, clips) != s;
}
// one sample: frame j of channel c of packet p, decoded value x; nothing happens at or behind lim
template <int DEPTH>
__device__ __forceinline__ void vf_sample(const DecodeArgs &A, const PcmModeArgs &F, uint32_t c, uint32_t p, uint32_t j,
                                          uint32_t lim, int32_t x)
{
    if (j >= lim) return;
    const float src = *vf_source(A, F, c, (uint64_t)p * A.frameSize + j);
    float d = 0.0f;
    if (F.dither) {  // uniform
        const uint64_t t = vf_origin(A, F, p) + j;
        uint32_t w[4];
        philox(t >> 1, c, F.dz, w);
        d = (t & 1) ? tpdf(w[2], w[3]) : tpdf(w[0], w[1]);
    }
    if (vf_differs<DEPTH>(src, d, x)) vf_mismatch(F, p, j);
}
// NF consecutive frames f0 .. of one channel, those in front of lim.  A whole group of four: the source as one 16-byte
// load where frameStride is 1 (4-byte alignment is all the input promises), the dither as dither4 spends it (two Philox
// calls per four frames, three where the first stream frame index is odd).  frameStride and the dither switch are
// uniform branches on kernel arguments, not template parameters: a template would double (twice) a mode that already
// adds an instantiation of every PCM-writing kernel, for a branch that costs one scalar compare per group.
template <int DEPTH, int NF>
__device__ __forceinline__ void vf_run(const DecodeArgs &A, const PcmModeArgs &F, uint32_t c, uint32_t p, uint32_t f0,
                                       uint32_t lim, const int32_t (&x)[NF])
{
    typedef float F4 __attribute__((ext_vector_type(4), aligned(4)));
    static_assert(NF % 4 == 0, "whole groups of four frames");
    if (f0 >= lim) return;
    const uint64_t j0 = (uint64_t)p * A.frameSize;
    const uint64_t t0 = F.dither ? vf_origin(A, F, p) : 0;
#pragma unroll
    for (int q = 0; q < NF / 4; q++) {
        const uint32_t f = f0 + 4 * q;
        if (f + 4 <= lim) {
            float s[4];
            if (F.frameStride == 1) {
                const F4 t = *(const F4 *)vf_source(A, F, c, j0 + f);
                s[0] = t.x, s[1] = t.y, s[2] = t.z, s[3] = t.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; e++) s[e] = *vf_source(A, F, c, j0 + f + e);
            }
            float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (F.dither) dither4(t0 + f, c, F.dz, z);
            uint32_t first = 4;
#pragma unroll
            for (int e = 3; e >= 0; e--)
                if (vf_differs<DEPTH>(s[e], z[e], x[4 * q + e])) first = (uint32_t)e;
            if (first < 4) vf_mismatch(F, p, f + first);
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) vf_sample<DEPTH>(A, F, c, p, f + e, lim, x[4 * q + e]);
        }
    }
}

// ---- int mode (alac_hip_decode_int) ----

// the value of a container: the decoded sample as alac_hip_decode stores it (the wrap of pcm_float), shifted to its place;
// the container is the low containerBytes bytes of this word (a right-justified sample arrives sign-extended in them)
template <int DEPTH>
__device__ __forceinline__ int32_t pcm_int(const PcmModeArgs &F, int32_t x)
{
    const int32_t s = DEPTH == 32 ? x : (int32_t)((uint32_t)x << (32 - DEPTH)) >> (32 - DEPTH);
    return (int32_t)((uint32_t)s << F.shift);
}
// index (in containers) of frame 0 of packet p of channel c
__device__ __forceinline__ uint64_t pi_origin(const DecodeArgs &A, const PcmModeArgs &F, uint32_t c, uint32_t p)
{
    return c * F.channelStride + (uint64_t)p * A.frameSize * F.frameStride;
}
// one container; the three bytes of a packed one as three byte stores (other lanes own the bytes on either side)
__device__ __forceinline__ void pi_store(const DecodeArgs &A, const PcmModeArgs &F, uint64_t at, int32_t v)
{
    if (F.containerBytes == 4) {
        ((int32_t *)A.pcmOut)[at] = v;
    } else if (F.containerBytes == 2) {
        ((int16_t *)A.pcmOut)[at] = (int16_t)v;
    } else {
        uint8_t *q = A.pcmOut + at * 3;
        q[0] = (uint8_t)v;
        q[1] = (uint8_t)(v >> 8);
        q[2] = (uint8_t)(v >> 16);
    }
}
// NF consecutive frames f0 .. of one channel, those in front of n.  A whole group of four where frameStride is 1: one 16-byte
// store of int32 containers, one 8-byte store of int16 containers (the container's own alignment is all the output promises);
// every other layout one store per sample.  Container width and strides are uniform branches on kernel arguments, for the
// reason vf_run gives.
template <int DEPTH, int NF>
__device__ __forceinline__ void pi_run(const DecodeArgs &A, const PcmModeArgs &F, uint32_t c, uint32_t p, uint32_t f0,
                                       uint32_t n, const int32_t (&x)[NF])
{
    typedef int32_t I4 __attribute__((ext_vector_type(4), aligned(4)));
    typedef int16_t S4 __attribute__((ext_vector_type(4), aligned(2)));
    static_assert(NF % 4 == 0, "whole groups of four frames");
    if (f0 >= n) return;
    const uint64_t at0 = pi_origin(A, F, c, p);
    const bool rows = F.frameStride == 1 && F.containerBytes != 3;
#pragma unroll
    for (int q = 0; q < NF / 4; q++) {
        const uint32_t f = f0 + 4 * q;
        if (rows && f + 4 <= n) {
            const int32_t v0 = pcm_int<DEPTH>(F, x[4 * q]), v1 = pcm_int<DEPTH>(F, x[4 * q + 1]);
            const int32_t v2 = pcm_int<DEPTH>(F, x[4 * q + 2]), v3 = pcm_int<DEPTH>(F, x[4 * q + 3]);
            if (F.containerBytes == 4) {
                const I4 t = {v0, v1, v2, v3};
                *(I4 *)((int32_t *)A.pcmOut + at0 + f) = t;
            } else {
                const S4 t = {(int16_t)v0, (int16_t)v1, (int16_t)v2, (int16_t)v3};
                *(S4 *)((int16_t *)A.pcmOut + at0 + f) = t;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (f + e < n) pi_store(A, F, at0 + (uint64_t)(f + e) * F.frameStride, pcm_int<DEPTH>(F, x[4 * q + e]));
        }
    }
}

// ---- what a sample branch calls: float mode stores, verify-float mode compares, int mode stores containers; lim =
// pcm_frames(...) of the packet ----
template <int DEPTH, PcmMode MODE>
__device__ __forceinline__ void pcm_sample_put(const DecodeArgs &A, const PcmModeArgs &F, uint32_t c, uint32_t p, uint32_t j,
                                              uint32_t lim, int32_t x)
{
    static_assert(pcm_by_sample(MODE), "a sample branch");
    if constexpr (MODE == kPcmFloat) pcm_float_row(A, c, p)[j] = pcm_float<DEPTH>(x);
    else if constexpr (MODE == kPcmInt) pi_store(A, F, pi_origin(A, F, c, p) + (uint64_t)j * F.frameStride, pcm_int<DEPTH>(F, x));
    else vf_sample<DEPTH>(A, F, c, p, j, lim, x);
}
template <int DEPTH, PcmMode MODE, int NF>
__device__ __forceinline__ void pcm_sample_run(const DecodeArgs &A, const PcmModeArgs &F, uint32_t c, uint32_t p, uint32_t f0,
                                              uint32_t lim, const int32_t (&x)[NF])
{
    static_assert(pcm_by_sample(MODE), "a sample branch");
    if constexpr (MODE == kPcmFloat) pcm_float_run<DEPTH>(pcm_float_row(A, c, p), f0, lim, x);
    else if constexpr (MODE == kPcmInt) pi_run<DEPTH>(A, F, c, p, f0, lim, x);
    else vf_run<DEPTH>(A, F, c, p, f0, lim, x);
}

// the frame that holds byte `at` of the expected PCM; a plain load first, so that a packet whose every frame differs
// (a damaged packet) costs one atomic per lane only while its minimum is still falling.  Inlined: as a called function it
// gave every verify kernel the call ABI — a 256-byte scratch frame, and the fused launch (whose entropy wave is the serial
// chain of a 10 000-packet pass) ran at twice the time of the decode pass
__device__ __forceinline__ void pcm_mismatch(const DecodeArgs &A, const uint8_t *at)
{
    const uint64_t off = (uint64_t)(at - A.pcmOut);
    const uint64_t packetBytes = (uint64_t)A.frameSize * A.frameBytes;
    const uint32_t p = (uint32_t)(off / packetBytes);
    const uint32_t frame = (uint32_t)((off - (uint64_t)p * packetBytes) / A.frameBytes);
    uint32_t *slot = A.firstMismatch + p;
    if (frame < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, frame);
}

// got = what the decoder produced, expected = the same bytes loaded from the caller's PCM (by value: registers only)
template <typename T>
__device__ __forceinline__ void pcm_compare(const DecodeArgs &A, const void *q, T expected, T got)
{
    constexpr int W = sizeof(T) >= 4 ? (int)(sizeof(T) / 4) : 1;
    static_assert(sizeof(T) < 4 || sizeof(T) % 4 == 0, "whole words or one sub-word field");
    uint32_t a[W] = {}, b[W] = {};
    __builtin_memcpy(a, &got, sizeof(T));
    __builtin_memcpy(b, &expected, sizeof(T));
    uint32_t at = ~0u;  // first differing byte of the field
#pragma unroll
    for (int k = W - 1; k >= 0; k--) {
        const uint32_t d = a[k] ^ b[k];
        if (d) at = 4u * (uint32_t)k + (uint32_t)__builtin_ctz(d) / 8u;
    }
    if (at != ~0u) pcm_mismatch(A, (const uint8_t *)q + at);
}

}  // namespace alacdev

#define PCM_PUT(MODE, A, ptr, value)                                                              \
    do {                                                                                          \
        static_assert(!alacdev::pcm_by_sample(MODE), "sample modes: the site's sample branch does the work"); \
        if constexpr ((MODE) == alacdev::kPcmVerify) alacdev::pcm_compare((A), (ptr), *(ptr), (value)); \
        else *(ptr) = (value);                                                                    \
    } while (0)
