// alac_verify.hpp — what the decoders' PCM store sites do: store (alac_hip_decode), verify (alac_hip_verify) or float
// (alac_hip_decode_float).
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
// float branch of its own in front of the packing, on the sample values it holds; PCM_PUT refuses to compile in float mode,
// so a site without one cannot slip through.  Where a lane holds four or more consecutive frames of a channel, the float
// branch writes them with 16-byte stores (pcm_float_run).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "alac_kernels.hpp"

namespace alacdev {

enum PcmMode : int { kPcmStore = 0, kPcmVerify = 1, kPcmFloat = 2 };

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
        static_assert((MODE) != alacdev::kPcmFloat, "float mode: the site stores floats itself"); \
        if constexpr ((MODE) == alacdev::kPcmVerify) alacdev::pcm_compare((A), (ptr), *(ptr), (value)); \
        else *(ptr) = (value);                                                                    \
    } while (0)
