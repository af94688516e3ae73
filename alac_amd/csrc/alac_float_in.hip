// alac_float_in.hip — float32 PCM -> the packed interleaved integer PCM alac_hip_encode reads (alac_hip_encode_float).
// One streaming pass in front of the unchanged encoder: quantize by the rule of include/alac_hip.h, pack, count clips;
// for alac_hip_encode_float_dither with TPDF dither from a counter-based generator in front of the rounding.
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_float_rule.hpp"
#include "alac_pcm_pack.hpp"

namespace alacdev {

// the ten round keys of a seed (the device side, philox, is in alac_float_rule.hpp)
void philox_round_keys(uint64_t seed, uint32_t (&roundKey)[10][2])
{
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; r++, k0 += kPhiloxW0, k1 += kPhiloxW1) roundKey[r][0] = k0, roundKey[r][1] = k1;
}

// One lane: 4 consecutive frames of one packet; a block: 1 024 frames of one packet (blocksPerPacket blocks per packet, a
// grid-stride loop over them).  Frames at or behind n = min(numSamples[p], frameSize) are not read and staged as zero.
// CH: 1 or 2 (the vector layouts, frameSize % 4 == 0, aligned strides and base: the host checks) or 0 (kFloatGeneral,
// a.channels at run time).  Clipped samples: per lane <= 4 * kMaxChannels; the wave sums them with one ballot per bit
// of the lane's count and adds the total to clipped[p] with one atomic (a block, hence a wave, lies in one packet).
// DITHER: every frame in front of n gets dz's dither for its stream frame index and channel (dither4: two Philox calls
// per channel and lane where the packet's origin is even); the staged zeros behind n stay zeros.  Without it dz is unused.
template <int DEPTH, int CH, int LAYOUT, bool DITHER>
__global__ __launch_bounds__(256) void k_float_to_pcm(FloatInArgs a, uint64_t blocksPerPacket, FloatDitherArgs dz)
{
    constexpr uint32_t BPS = bytes_per_sample(DEPTH);
    constexpr int CNT_BITS = CH == 1 ? 3 : (CH == 2 ? 4 : 6);  // bits of a lane's clip count: <= 4, 8, 32
    const uint64_t totalBlocks = (uint64_t)a.numPackets * blocksPerPacket;
    for (uint64_t vb = blockIdx.x; vb < totalBlocks; vb += gridDim.x) {
        const uint32_t p = (uint32_t)(vb / blocksPerPacket);
        const uint32_t i0 = (uint32_t)(vb % blocksPerPacket) * 1024u + threadIdx.x * 4u;
        const uint32_t fs = a.frameSize;
        uint32_t n = a.numSamples ? a.numSamples[p] : fs;
        n = n < fs ? n : fs;
        const uint64_t f0 = (uint64_t)p * fs + i0;  // frame index of the lane's first frame in the batch
        uint32_t clips = 0;
        uint64_t t0 = 0;  // stream frame index of the lane's first frame
        if constexpr (DITHER) t0 = (dz.origin ? dz.origin[p] : (uint64_t)p * fs) + i0;
        if constexpr (LAYOUT == kFloatGeneral && DITHER) {
            const uint32_t C = a.channels;
            for (uint32_t c = 0; c < C && i0 < fs; c++) {
                float z[4];
                dither4(t0, c, dz, z);
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t i = i0 + k;
                    if (i < fs) {
                        const bool live = i < n;
                        const float x = live ? a.in[c * a.channelStride + (f0 + k) * a.frameStride] : 0.0f;
                        store_sample<DEPTH>(a.pcm + ((f0 + k) * C + c) * BPS,
                                            quantize_dithered<DEPTH>(x, live ? z[k] : 0.0f, clips));
                    }
                }
            }
        } else if constexpr (LAYOUT == kFloatGeneral) {
            const uint32_t C = a.channels;
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t i = i0 + k;
                if (i >= fs) break;
                uint8_t *dst = a.pcm + (f0 + k) * C * BPS;
                for (uint32_t c = 0; c < C; c++) {
                    const float x = i < n ? a.in[c * a.channelStride + (f0 + k) * a.frameStride] : 0.0f;
                    store_sample<DEPTH>(dst + c * BPS, quantize<DEPTH>(x, clips));
                }
            }
        } else if (i0 < fs) {  // vector layouts: frameSize % 4 == 0, so the lane's 4 frames lie in the packet
            float x[CH][4];
            if (i0 + 4 <= n) {
                if constexpr (LAYOUT == kFloatPlanar) {
#pragma unroll
                    for (int c = 0; c < CH; c++) {
                        const float4 v = *(const float4 *)(a.in + c * a.channelStride + f0);
                        x[c][0] = v.x, x[c][1] = v.y, x[c][2] = v.z, x[c][3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < CH; q++) {
                        const float4 v = *(const float4 *)(a.in + f0 * CH + 4 * q);
                        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                        for (int k = 0; k < 4; k++) x[(4 * q + k) % CH][(4 * q + k) / CH] = e[k];
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < CH; c++)
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        x[c][k] = i0 + k < n ? a.in[c * a.channelStride + (f0 + k) * a.frameStride] : 0.0f;
            }
            int32_t s[4 * CH];
            if constexpr (DITHER) {
#pragma unroll
                for (int c = 0; c < CH; c++) {
                    float z[4];
                    dither4(t0, c, dz, z);
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        s[k * CH + c] = quantize_dithered<DEPTH>(x[c][k], i0 + k < n ? z[k] : 0.0f, clips);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
#pragma unroll
                    for (int c = 0; c < CH; c++) s[k * CH + c] = quantize<DEPTH>(x[c][k], clips);
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
}

template <int DEPTH, bool DITHER>
static hipError_t launch_depth(const FloatInArgs &a, const FloatDitherArgs &dz, FloatLayout layout, dim3 grid, uint64_t bpp,
                               hipStream_t st)
{
    if (layout == kFloatGeneral) return launch_kernel(k_float_to_pcm<DEPTH, 0, kFloatGeneral, DITHER>, grid, dim3(256), st, a, bpp, dz);
    if (a.channels == 1) return launch_kernel(k_float_to_pcm<DEPTH, 1, kFloatPlanar, DITHER>, grid, dim3(256), st, a, bpp, dz);
    if (layout == kFloatPlanar) return launch_kernel(k_float_to_pcm<DEPTH, 2, kFloatPlanar, DITHER>, grid, dim3(256), st, a, bpp, dz);
    return launch_kernel(k_float_to_pcm<DEPTH, 2, kFloatInterleaved, DITHER>, grid, dim3(256), st, a, bpp, dz);
}

hipError_t launch_float_to_pcm(uint32_t depth, const FloatInArgs &a, hipStream_t st, const FloatDitherArgs *dither)
{
    if (dither && depth != 16 && depth != 20 && depth != 24) return hipErrorInvalidValue;  // no dither at 32 bits
    if (a.numPackets == 0) return hipSuccess;
    if (a.clipped) ALAC_TRY(hipMemsetAsync(a.clipped, 0, (uint64_t)a.numPackets * 4, st));
    // the vector paths: whole 4-frame groups inside a packet, 16-byte aligned float4 loads at every group
    const FloatLayout layout =
        a.frameSize % 4 == 0 ? float_layout(a.in, a.channels, a.channelStride, a.frameStride) : kFloatGeneral;
    const uint64_t bpp = ((uint64_t)a.frameSize + 1023) / 1024;
    const uint64_t blocks = (uint64_t)a.numPackets * bpp;
    const dim3 grid((uint32_t)(blocks < (1u << 22) ? blocks : (1u << 22)));
    if (dither) {
        switch (depth) {
        case 16: return launch_depth<16, true>(a, *dither, layout, grid, bpp, st);
        case 20: return launch_depth<20, true>(a, *dither, layout, grid, bpp, st);
        default: return launch_depth<24, true>(a, *dither, layout, grid, bpp, st);
        }
    }
    const FloatDitherArgs none = {};
    switch (depth) {
    case 16: return launch_depth<16, false>(a, none, layout, grid, bpp, st);
    case 20: return launch_depth<20, false>(a, none, layout, grid, bpp, st);
    case 24: return launch_depth<24, false>(a, none, layout, grid, bpp, st);
    default: return launch_depth<32, false>(a, none, layout, grid, bpp, st);
    }
}

}  // namespace alacdev
