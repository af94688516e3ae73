// alac_pcm_walk.hpp — the walk of the conversion passes in front of the encoder (k_float_to_pcm, alac_float_in.hip, and
// k_pcm_requantize, alac_pcm_in.hip): blocks and packets, the three layouts, pack and store, the clip count.  What a source
// format adds is its policy (loads and the rule that turns 4 samples of a channel into 4 staged integers), its kernel and its
// launcher.  DESIGN.md section 20.
#pragma once
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_pcm_pack.hpp"

namespace alacdev {

// One lane: 4 consecutive frames of one packet; a block: 1 024 frames of one packet (blocksPerPacket blocks per packet, a
// grid-stride loop over them).  Frames at or behind n = min(numSamples[p], frameSize) are not read and staged as zero.
// CH: 1 or 2 (the vector layouts of pcm_in_layout, frameSize % 4 == 0: the host checks) or 0 (kFloatGeneral, a.channels at
// run time, one load and one store per sample, channel by channel: a channel's 4 loads go out in front of its 4 stores, so
// pcm must not overlap the source).  Clipped samples: per lane <= 4 * kMaxChannels; the wave sums them with one ballot per
// bit of the lane's count and adds the total to clipped[p] with one atomic (a block, hence a wave, lies in one packet).
// Src: Elem, the type of a sample as loaded; kDither; load1(index) and load_run<N>(index, e), N consecutive samples from an
// index that pcm_in_layout's alignment covers; convert4(x, live, t0, c, dz, s, clips): the 4 samples x of channel c at stream
// frames t0 .. t0 + 3; one that is not live lies behind n, is zero and gets no dither.
template <int DEPTH, int CH, int LAYOUT, typename Src, typename Args>
__device__ __forceinline__ void pcm_walk(const Src &src, const Args &a, uint64_t blocksPerPacket, const FloatDitherArgs &dz)
{
    using Elem = typename Src::Elem;
    constexpr uint32_t BPS = bytes_per_sample(DEPTH);
    constexpr int CNT_BITS = CH == 1 ? 3 : (CH == 2 ? 4 : 6);  // bits of a lane's clip count: <= 4, 8, 32
    const uint64_t totalBlocks = (uint64_t)a.numPackets * blocksPerPacket;
    for (uint64_t vb = blockIdx.x; vb < totalBlocks; vb += gridDim.x) {
        const uint32_t p = (uint32_t)(vb / blocksPerPacket);
        const uint32_t i0 = (uint32_t)(vb % blocksPerPacket) * 1024u + threadIdx.x * 4u;
        const uint32_t fs = a.frameSize;
        uint32_t n = a.numSamples ? a.numSamples[p] : fs;
        n = n < fs ? n : fs;
        const bool live[4] = {i0 < n, i0 + 1 < n, i0 + 2 < n, i0 + 3 < n};  // which of the lane's frames lie in front of n
        const uint64_t f0 = (uint64_t)p * fs + i0;  // frame index of the lane's first frame in the batch
        uint32_t clips = 0;
        uint64_t t0 = 0;  // stream frame index of the lane's first frame
        if constexpr (Src::kDither) t0 = (dz.origin ? dz.origin[p] : (uint64_t)p * fs) + i0;
        if constexpr (LAYOUT == kFloatGeneral) {
            const uint32_t C = a.channels;
            for (uint32_t c = 0; c < C && i0 < fs; c++) {
                Elem x[4];
                int32_t s[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; k++)
                    x[k] = live[k] ? src.load1(c * a.channelStride + (f0 + k) * a.frameStride) : Elem(0);
                src.convert4(x, live, t0, c, dz, s, clips);
#pragma unroll
                for (uint32_t k = 0; k < 4; k++)
                    if (i0 + k < fs) store_sample<DEPTH>(a.pcm + ((f0 + k) * C + c) * BPS, s[k]);
            }
        } else if (i0 < fs) {  // vector layouts: frameSize % 4 == 0, so the lane's 4 frames lie in the packet
            Elem x[CH][4];
            if (i0 + 4 <= n) {
                if constexpr (LAYOUT == kFloatPlanar) {
#pragma unroll
                    for (int c = 0; c < CH; c++) src.load_run(c * a.channelStride + f0, x[c]);
                } else {
                    Elem e[4 * CH];
                    src.load_run(f0 * CH, e);
#pragma unroll
                    for (int j = 0; j < 4 * CH; j++) x[j % CH][j / CH] = e[j];
                }
            } else {
#pragma unroll
                for (int c = 0; c < CH; c++)
#pragma unroll
                    for (uint32_t k = 0; k < 4; k++)
                        x[c][k] = live[k] ? src.load1(c * a.channelStride + (f0 + k) * a.frameStride) : Elem(0);
            }
            int32_t s[4 * CH];
#pragma unroll
            for (int c = 0; c < CH; c++) {
                int32_t sc[4];
                src.convert4(x[c], live, t0, c, dz, sc, clips);
#pragma unroll
                for (int k = 0; k < 4; k++) s[k * CH + c] = sc[k];
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

// the launch of a conversion kernel: zeroes the clip counts, then 1 024 frames per block.  layout: what pcm_in_layout says of
// the source; a frame size that is no multiple of 4 leaves no whole 4-frame groups inside a packet, hence the general layout.
// launch(CH, LAYOUT, grid, blocksPerPacket) starts the kernel of that pair.
template <typename Args, typename Launch>
inline hipError_t launch_pcm_walk(const Args &a, FloatLayout layout, hipStream_t st, Launch launch)
{
    if (a.numPackets == 0) return hipSuccess;
    if (a.clipped) ALAC_TRY(hipMemsetAsync(a.clipped, 0, (uint64_t)a.numPackets * 4, st));
    const uint64_t bpp = ((uint64_t)a.frameSize + 1023) / 1024;
    const uint64_t blocks = (uint64_t)a.numPackets * bpp;
    const dim3 grid((uint32_t)(blocks < (1u << 22) ? blocks : (1u << 22)));
    return dispatch_layout(a.frameSize % 4 == 0 ? layout : kFloatGeneral, a.channels,
                           [&](auto ch, auto lay) { return launch(ch, lay, grid, bpp); });
}

}  // namespace alacdev
