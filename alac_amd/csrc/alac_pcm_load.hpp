// alac_pcm_load.hpp — how the integer passes (alac_pcm_in.hip, the integer source of pcm_walk, alac_pcm_walk.hpp; and
// alac_int_probe.hip, the integer rule of probe_walk, alac_probe_walk.hpp) take containers out of memory: one container by
// its index, and a run of consecutive ones with vector loads.  The layouts that allow the runs: pcm_in_layout
// (alac_kernels.hpp).
#pragma once
#include "alac_dev.hpp"

namespace alacdev {

// one container, sign-extended
template <int CB>
__device__ __forceinline__ int32_t load_container(const void *in, uint64_t idx)
{
    if constexpr (CB == 2) {
        return ((const int16_t *)in)[idx];
    } else if constexpr (CB == 4) {
        return ((const int32_t *)in)[idx];
    } else {
        const uint8_t *b = (const uint8_t *)in + idx * 3;
        return (int32_t)((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16)) << 8 >> 8;
    }
}

// N consecutive containers (N a multiple of 4) at p, which is aligned to 16 bytes (CB 4), 8 (CB 2) or 4 (CB 3)
template <int CB, int N>
__device__ __forceinline__ void load_run(const uint8_t *p, int32_t (&e)[N])
{
    if constexpr (CB == 4) {
#pragma unroll
        for (int q = 0; q < N / 4; q++) {
            const int4 v = ((const int4 *)p)[q];
            e[4 * q] = v.x, e[4 * q + 1] = v.y, e[4 * q + 2] = v.z, e[4 * q + 3] = v.w;
        }
    } else if constexpr (CB == 2) {
#pragma unroll
        for (int q = 0; q < N / 4; q++) {
            const uint2 v = ((const uint2 *)p)[q];
            e[4 * q] = (int16_t)v.x, e[4 * q + 1] = (int32_t)v.x >> 16;
            e[4 * q + 2] = (int16_t)v.y, e[4 * q + 3] = (int32_t)v.y >> 16;
        }
    } else {
        uint32_t w[3 * N / 4];
#pragma unroll
        for (int q = 0; q < 3 * N / 4; q++) w[q] = ((const uint32_t *)p)[q];
#pragma unroll
        for (int q = 0; q < N / 4; q++) {  // the inverse of pack_dwords' 3-byte case
            e[4 * q] = (int32_t)(w[3 * q] << 8) >> 8;
            e[4 * q + 1] = (int32_t)(((w[3 * q] >> 24) | (w[3 * q + 1] << 8)) << 8) >> 8;
            e[4 * q + 2] = (int32_t)(((w[3 * q + 1] >> 16) | (w[3 * q + 2] << 16)) << 8) >> 8;
            e[4 * q + 3] = (int32_t)w[3 * q + 2] >> 8;
        }
    }
}

}  // namespace alacdev
