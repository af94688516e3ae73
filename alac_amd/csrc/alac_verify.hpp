// alac_verify.hpp — the store sites of the decoders' PCM in verify mode (alac_hip_verify).
//
// Every kernel that writes PCM writes it through PCM_PUT(VERIFY, A, ptr, value).  With VERIFY = false that is the plain store
// `*ptr = value` it always was, through the site's own pointer type (its alignment included: a template would deduce the
// canonical vector type and assume 16-byte alignment), so the instantiation the decode entry point launches is unchanged.
// With VERIFY = true, DecodeArgs::pcmOut is the caller's expected PCM in the layout alac_hip_decode writes: the site loads
// the same bytes through the same pointer (a load as wide as the store), and where they differ lowers firstMismatch[packet]
// to the frame of the first differing byte.  Nothing is stored, so a verify pass reads the expected PCM where a decode
// pass writes the decoded PCM.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "alac_kernels.hpp"

namespace alacdev {

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

#define PCM_PUT(VERIFY, A, ptr, value)                                    \
    do {                                                                  \
        if constexpr (VERIFY) alacdev::pcm_compare((A), (ptr), *(ptr), (value)); \
        else *(ptr) = (value);                                            \
    } while (0)
