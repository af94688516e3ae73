// alac_float_in.hip — float32 PCM -> the packed interleaved integer PCM alac_hip_encode reads (alac_hip_encode_float).
// One streaming pass in front of the unchanged encoder: quantize by the rule of include/alac_hip.h, pack, count clips;
// for alac_hip_encode_float_dither with TPDF dither from a counter-based generator in front of the rounding.
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_float_rule.hpp"
#include "alac_pcm_walk.hpp"

namespace alacdev {

// the ten round keys of a seed (the device side, philox, is in alac_float_rule.hpp)
void philox_round_keys(uint64_t seed, uint32_t (&roundKey)[10][2])
{
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; r++, k0 += kPhiloxW0, k1 += kPhiloxW1) roundKey[r][0] = k0, roundKey[r][1] = k1;
}

// the float32 source of pcm_walk (alac_pcm_walk.hpp): the rule of alac_float_rule.hpp.  DITHER: every frame in front of n
// gets dz's dither for its stream frame index and channel (dither4: two Philox calls per channel and lane where the packet's
// origin is even); the staged zeros behind n stay zeros.  Without it dz is unused.
template <int DEPTH, bool DITHER>
struct FloatSrc {
    using Elem = float;
    static constexpr bool kDither = DITHER;
    const float *in;

    __device__ __forceinline__ float load1(uint64_t idx) const { return in[idx]; }
    template <int N>
    __device__ __forceinline__ void load_run(uint64_t idx, float (&e)[N]) const
    {
#pragma unroll
        for (int q = 0; q < N / 4; q++) {
            const float4 v = ((const float4 *)(in + idx))[q];
            e[4 * q] = v.x, e[4 * q + 1] = v.y, e[4 * q + 2] = v.z, e[4 * q + 3] = v.w;
        }
    }
    __device__ __forceinline__ void convert4(const float (&x)[4], const bool (&live)[4], uint64_t t0, uint32_t c,
                                             const FloatDitherArgs &dz, int32_t (&s)[4], uint32_t &clips) const
    {
        if constexpr (DITHER) {
            float z[4];
            dither4(t0, c, dz, z);
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) s[k] = quantize_dithered<DEPTH>(x[k], live[k] ? z[k] : 0.0f, clips);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) s[k] = quantize<DEPTH>(x[k], clips);
        }
    }
};

// The dithered vector instantiations (DITHER, CH 1 or 2) stay on the loop they had before pcm_walk: on the walker the compiler
// schedules their Philox chains otherwise and they time 1 .. 3 % slower (profiles/input_walkers/ab.md).  pcm_walk's vector
// path, with the float rule written in; change the two together.
template <int DEPTH, int CH, int LAYOUT, bool DITHER>
__global__ __launch_bounds__(256) void k_float_to_pcm(FloatInArgs a, uint64_t blocksPerPacket, FloatDitherArgs dz)
{
    if constexpr (DITHER && LAYOUT != kFloatGeneral) {
        constexpr uint32_t BPS = bytes_per_sample(DEPTH);
        constexpr int CNT_BITS = CH == 1 ? 3 : 4;  // bits of a lane's clip count: <= 4, 8
        const uint64_t totalBlocks = (uint64_t)a.numPackets * blocksPerPacket;
        for (uint64_t vb = blockIdx.x; vb < totalBlocks; vb += gridDim.x) {
            const uint32_t p = (uint32_t)(vb / blocksPerPacket);
            const uint32_t i0 = (uint32_t)(vb % blocksPerPacket) * 1024u + threadIdx.x * 4u;
            const uint32_t fs = a.frameSize;
            uint32_t n = a.numSamples ? a.numSamples[p] : fs;
            n = n < fs ? n : fs;
            const uint64_t f0 = (uint64_t)p * fs + i0;
            uint32_t clips = 0;
            const uint64_t t0 = (dz.origin ? dz.origin[p] : (uint64_t)p * fs) + i0;
            if (i0 < fs) {
                const FloatSrc<DEPTH, true> src = {a.in};
                float x[CH][4];
                if (i0 + 4 <= n) {
                    if constexpr (LAYOUT == kFloatPlanar) {
#pragma unroll
                        for (int c = 0; c < CH; c++) src.load_run(c * a.channelStride + f0, x[c]);
                    } else {
                        float e[4 * CH];
                        src.load_run(f0 * CH, e);
#pragma unroll
                        for (int j = 0; j < 4 * CH; j++) x[j % CH][j / CH] = e[j];
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < CH; c++)
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            x[c][k] = i0 + k < n ? a.in[c * a.channelStride + (f0 + k) * a.frameStride] : 0.0f;
                }
                int32_t s[4 * CH];
#pragma unroll
                for (int c = 0; c < CH; c++) {
                    float z[4];
                    dither4(t0, c, dz, z);
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        s[k * CH + c] = quantize_dithered<DEPTH>(x[c][k], i0 + k < n ? z[k] : 0.0f, clips);
                }
                uint32_t w[CH * BPS];
                pack_dwords<DEPTH, 4 * CH>(s, w);
                store_dwords<CH * BPS>(a.pcm + f0 * (CH * BPS), w);
            }
            if (a.clipped) {
                uint32_t total = 0;
#pragma unroll
                for (int b = 0; b < CNT_BITS; b++) total += (uint32_t)__popcll(__ballot((clips >> b) & 1u)) << b;
                if ((threadIdx.x & 63) == 0 && total) atomicAdd(a.clipped + p, total);
            }
        }
    } else {
        pcm_walk<DEPTH, CH, LAYOUT>(FloatSrc<DEPTH, DITHER>{a.in}, a, blocksPerPacket, dz);
    }
}

template <int DEPTH, bool DITHER>
static hipError_t launch_depth(const FloatInArgs &a, const FloatDitherArgs &dz, hipStream_t st)
{
    const FloatLayout layout = pcm_in_layout(a.in, 4, a.channels, a.channelStride, a.frameStride);
    return launch_pcm_walk(a, layout, st, [&](auto ch, auto lay, dim3 grid, uint64_t bpp) {
        return launch_kernel(k_float_to_pcm<DEPTH, decltype(ch)::value, decltype(lay)::value, DITHER>, grid, dim3(256), st, a, bpp, dz);
    });
}

hipError_t launch_float_to_pcm(uint32_t depth, const FloatInArgs &a, hipStream_t st, const FloatDitherArgs *dither)
{
    if (dither && depth != 16 && depth != 20 && depth != 24) return hipErrorInvalidValue;  // no dither at 32 bits
    const FloatDitherArgs none = {};
    const FloatDitherArgs &dz = dither ? *dither : none;
    switch (depth) {
    case 16: return dither ? launch_depth<16, true>(a, dz, st) : launch_depth<16, false>(a, dz, st);
    case 20: return dither ? launch_depth<20, true>(a, dz, st) : launch_depth<20, false>(a, dz, st);
    case 24: return dither ? launch_depth<24, true>(a, dz, st) : launch_depth<24, false>(a, dz, st);
    default: return launch_depth<32, false>(a, dz, st);
    }
}

}  // namespace alacdev
