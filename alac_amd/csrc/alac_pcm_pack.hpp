// alac_pcm_pack.hpp — integer samples -> the packed interleaved little-endian PCM alac_hip_encode reads, as device code.
// The stores of pcm_walk (alac_pcm_walk.hpp), the one walk of the two conversion passes in front of the encoder:
// alac_float_in.hip (float32 sources) and alac_pcm_in.hip (integer sources).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "alac_dev.hpp"

namespace alacdev {

// a sample as it sits in its container: 20-bit left-justified in 3 bytes (task_load / load_sample read it back >> 4)
template <int DEPTH>
__device__ __forceinline__ uint32_t container(int32_t s)
{
    return DEPTH == 20 ? (uint32_t)s << 4 : (uint32_t)s;
}

// N interleaved samples (N a multiple of 4) -> their N * bytes_per_sample(DEPTH) / 4 little-endian dwords
template <int DEPTH, int N>
__device__ __forceinline__ void pack_dwords(const int32_t (&s)[N], uint32_t (&w)[N * (int)bytes_per_sample(DEPTH) / 4])
{
    if constexpr (DEPTH == 16) {
#pragma unroll
        for (int k = 0; k < N / 2; k++) w[k] = ((uint32_t)s[2 * k] & 0xffffu) | ((uint32_t)s[2 * k + 1] << 16);
    } else if constexpr (DEPTH == 32) {
#pragma unroll
        for (int k = 0; k < N; k++) w[k] = (uint32_t)s[k];
    } else {
#pragma unroll
        for (int q = 0; q < N / 4; q++) {
            const uint32_t v0 = container<DEPTH>(s[4 * q]) & 0xffffffu, v1 = container<DEPTH>(s[4 * q + 1]) & 0xffffffu;
            const uint32_t v2 = container<DEPTH>(s[4 * q + 2]) & 0xffffffu, v3 = container<DEPTH>(s[4 * q + 3]) & 0xffffffu;
            w[3 * q] = v0 | (v1 << 24);
            w[3 * q + 1] = (v1 >> 8) | (v2 << 16);
            w[3 * q + 2] = (v2 >> 16) | (v3 << 8);
        }
    }
}

// W dwords to dst, as 16-byte stores where W allows it, else 8-byte, else dword (dst is aligned to 4 * W bytes' largest
// power-of-two divisor up to 16: a whole 4-frame group at a 4-frame-aligned position of the 256-byte aligned stage)
template <int W>
__device__ __forceinline__ void store_dwords(uint8_t *dst, const uint32_t (&w)[W])
{
    if constexpr (W % 4 == 0) {
#pragma unroll
        for (int k = 0; k < W / 4; k++) ((uint4 *)dst)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    } else if constexpr (W % 2 == 0) {
#pragma unroll
        for (int k = 0; k < W / 2; k++) ((uint2 *)dst)[k] = make_uint2(w[2 * k], w[2 * k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < W; k++) ((uint32_t *)dst)[k] = w[k];
    }
}

template <int DEPTH>
__device__ __forceinline__ void store_sample(uint8_t *dst, int32_t s)
{
    if constexpr (DEPTH == 16) {
        *(uint16_t *)dst = (uint16_t)s;
    } else if constexpr (DEPTH == 32) {
        *(uint32_t *)dst = (uint32_t)s;
    } else {
        const uint32_t v = container<DEPTH>(s);
        dst[0] = (uint8_t)v;
        dst[1] = (uint8_t)(v >> 8);
        dst[2] = (uint8_t)(v >> 16);
    }
}

}  // namespace alacdev
