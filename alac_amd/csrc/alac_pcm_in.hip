// alac_pcm_in.hip — integer PCM of any layout, container and depth -> the packed interleaved integer PCM alac_hip_encode
// reads (alac_hip_pcm_requantize, the conversion pass of alac_hip_encode_int).  One streaming pass in front of the unchanged
// encoder: take the sample out of its container, widen it or reduce it by the integer rule of include/alac_hip.h (round
// half to even, optionally TPDF dither from the generator of alac_float_rule.hpp), pack, count clips.
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_float_rule.hpp"
#include "alac_pcm_pack.hpp"
#include "alac_pcm_load.hpp"

namespace alacdev {

// what a call's source and target depths come to, the same for every sample (scalars)
struct PcmInRule {
    uint32_t rsh;     // left-justified: 8 * container bytes - S, the shift that takes the sample out; else 0
    int32_t lo, hi;   // [-2^(S-1), 2^(S-1) - 1]: what a right-justified container is saturated to
    uint32_t lsh, D;  // b >= S: r = s << lsh and D = 0; b < S: D = S - b
};

template <int DEPTH, int CB>
__device__ __forceinline__ PcmInRule pcm_in_rule(const PcmInArgs &a)
{
    const uint32_t S = a.srcBits;
    PcmInRule r;
    r.rsh = a.leftJustified ? 8u * CB - S : 0u;
    r.hi = (int32_t)(0x7fffffffu >> (32u - S));
    r.lo = ~r.hi;
    r.lsh = DEPTH >= S ? DEPTH - S : 0u;
    r.D = DEPTH >= S ? 0u : S - DEPTH;
    return r;
}

// the rule: container v (0 behind the packet's frames, with k = 0) -> the staged sample at DEPTH bits
template <int DEPTH, bool DITHER>
__device__ __forceinline__ int32_t requantize(int32_t v, int32_t k, const PcmInRule &R, uint32_t &clips)
{
    constexpr int32_t kMax = (int32_t)((1ull << (DEPTH - 1)) - 1), kMin = -kMax - 1;
    const int32_t s0 = v >> R.rsh;
    const int32_t s = min(max(s0, R.lo), R.hi);  // a left-justified sample lies inside: only right-justified ones saturate
    int32_t r;
    if constexpr (DITHER) {  // D > 0: the launcher refuses dither where nothing is rounded
        // acc = s * 2^(24 - D) + k without 64-bit words: s = (s >> D) * 2^D + low bits, so acc = (s >> D) * 2^24 + f with
        // f = (low bits << (24 - D)) + k in (-2^24, 2^25) and q = acc >> 24 = (s >> D) + (f >> 24).  The rounding as one
        // biased shift: floor((acc + 2^23 - 1 + (q & 1)) / 2^24) is q below a half, q + 1 above it and q + (q & 1) at it.
        // (The kernel is bound by its integer instructions under dither, two thirds of them Philox's: every one counts.)
        const int32_t q0 = s >> R.D;
        const int32_t f = (int32_t)(((uint32_t)s & ((1u << R.D) - 1u)) << (24u - R.D)) + k;
        r = q0 + ((f + 0x7fffff + ((q0 + (f >> 24)) & 1)) >> 24);
    } else if (R.D == 0) {
        return clips += s != s0 ? 1u : 0u, (int32_t)((uint32_t)s << R.lsh);
    } else {  // k = 0: acc / 2^24 = s / 2^D, the same quotient and the same comparison of the remainder with a half
        const int32_t q = s >> R.D;
        const uint32_t rem = (uint32_t)s & ((1u << R.D) - 1u), half = 1u << (R.D - 1u);
        r = q + ((rem > half || (rem == half && (q & 1))) ? 1 : 0);
    }
    const int32_t out = min(max(r, kMin), kMax);
    clips += (s != s0 || out != r) ? 1u : 0u;
    return out;
}

// The geometry of k_float_to_pcm (alac_float_in.hip).  One lane: 4 consecutive frames of one packet; a block: 1 024 frames
// of one packet (blocksPerPacket blocks per packet, a grid-stride loop over them).  Frames at or behind n =
// min(numSamples[p], frameSize) are not read and staged as zero, without dither.  CB: the container's bytes.  CH: 1 or 2
// (the vector layouts of pcm_in_layout, frameSize % 4 == 0: the host checks) or 0 (kFloatGeneral, a.channels at run time,
// one load per sample).  Clipped samples: per lane <= 4 * kMaxChannels; the wave sums them with one ballot per bit of the
// lane's count and adds the total to clipped[p] with one atomic (a block, hence a wave, lies in one packet).
template <int DEPTH, int CB, int CH, int LAYOUT, bool DITHER>
__global__ __launch_bounds__(256) void k_pcm_requantize(PcmInArgs a, uint64_t blocksPerPacket, FloatDitherArgs dz)
{
    constexpr uint32_t BPS = bytes_per_sample(DEPTH);
    constexpr int CNT_BITS = CH == 1 ? 3 : (CH == 2 ? 4 : 6);  // bits of a lane's clip count: <= 4, 8, 32
    const PcmInRule R = pcm_in_rule<DEPTH, CB>(a);
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
        if constexpr (LAYOUT == kFloatGeneral) {
            const uint32_t C = a.channels;
            for (uint32_t c = 0; c < C && i0 < fs; c++) {
                int32_t z[4] = {0, 0, 0, 0};
                if constexpr (DITHER) dither4_k(t0, c, dz, z);
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t i = i0 + k;
                    if (i < fs) {
                        const bool live = i < n;
                        const int32_t v = live ? load_container<CB>(a.in, c * a.channelStride + (f0 + k) * a.frameStride) : 0;
                        store_sample<DEPTH>(a.pcm + ((f0 + k) * C + c) * BPS,
                                            requantize<DEPTH, DITHER>(v, live ? z[k] : 0, R, clips));
                    }
                }
            }
        } else if (i0 < fs) {  // vector layouts: frameSize % 4 == 0, so the lane's 4 frames lie in the packet
            int32_t v[CH][4];
            if (i0 + 4 <= n) {
                if constexpr (LAYOUT == kFloatPlanar) {
#pragma unroll
                    for (int c = 0; c < CH; c++) load_run<CB, 4>((const uint8_t *)a.in + (c * a.channelStride + f0) * CB, v[c]);
                } else {
                    int32_t e[4 * CH];
                    load_run<CB, 4 * CH>((const uint8_t *)a.in + f0 * (CH * CB), e);
#pragma unroll
                    for (int j = 0; j < 4 * CH; j++) v[j % CH][j / CH] = e[j];
                }
            } else {
#pragma unroll
                for (int c = 0; c < CH; c++)
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        v[c][k] = i0 + k < n ? load_container<CB>(a.in, c * a.channelStride + (f0 + k) * a.frameStride) : 0;
            }
            int32_t s[4 * CH];
#pragma unroll
            for (int c = 0; c < CH; c++) {
                int32_t z[4] = {0, 0, 0, 0};
                if constexpr (DITHER) dither4_k(t0, c, dz, z);
#pragma unroll
                for (int k = 0; k < 4; k++)
                    s[k * CH + c] = requantize<DEPTH, DITHER>(v[c][k], i0 + k < n ? z[k] : 0, R, clips);
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

template <int DEPTH, int CB, bool DITHER>
static hipError_t launch_layout(const PcmInArgs &a, const FloatDitherArgs &dz, FloatLayout layout, dim3 grid, uint64_t bpp,
                                hipStream_t st)
{
    if (layout == kFloatGeneral)
        return launch_kernel(k_pcm_requantize<DEPTH, CB, 0, kFloatGeneral, DITHER>, grid, dim3(256), st, a, bpp, dz);
    if (a.channels == 1) return launch_kernel(k_pcm_requantize<DEPTH, CB, 1, kFloatPlanar, DITHER>, grid, dim3(256), st, a, bpp, dz);
    if (layout == kFloatInterleaved)
        return launch_kernel(k_pcm_requantize<DEPTH, CB, 2, kFloatInterleaved, DITHER>, grid, dim3(256), st, a, bpp, dz);
    if constexpr (CB != 3)  // pcm_in_layout names no planar layout of two rows of packed 3-byte containers
        return launch_kernel(k_pcm_requantize<DEPTH, CB, 2, kFloatPlanar, DITHER>, grid, dim3(256), st, a, bpp, dz);
    return hipErrorInvalidValue;
}

// dither is a reduction's: 3- and 4-byte containers (a 2-byte one holds 16 bits, the smallest target)
template <int DEPTH>
static hipError_t launch_container(const PcmInArgs &a, const FloatDitherArgs *dz, FloatLayout layout, dim3 grid, uint64_t bpp,
                                   hipStream_t st)
{
    const FloatDitherArgs none = {};
    if constexpr (DEPTH != 32) {
        if (dz && a.containerBytes == 3) return launch_layout<DEPTH, 3, true>(a, *dz, layout, grid, bpp, st);
        if (dz && a.containerBytes == 4) return launch_layout<DEPTH, 4, true>(a, *dz, layout, grid, bpp, st);
    }
    if (dz) return hipErrorInvalidValue;
    switch (a.containerBytes) {
    case 2: return launch_layout<DEPTH, 2, false>(a, none, layout, grid, bpp, st);
    case 3: return launch_layout<DEPTH, 3, false>(a, none, layout, grid, bpp, st);
    default: return launch_layout<DEPTH, 4, false>(a, none, layout, grid, bpp, st);
    }
}

hipError_t launch_pcm_requantize(uint32_t depth, const PcmInArgs &a, hipStream_t st, const FloatDitherArgs *dither)
{
    const uint32_t S = a.srcBits, CB = a.containerBytes;
    if ((depth != 16 && depth != 20 && depth != 24 && depth != 32) || (S != 16 && S != 20 && S != 24 && S != 32) ||
        CB < 2 || CB > 4 || S > 8 * CB || (dither && depth >= S))
        return hipErrorInvalidValue;
    if (a.numPackets == 0) return hipSuccess;
    if (a.clipped) ALAC_TRY(hipMemsetAsync(a.clipped, 0, (uint64_t)a.numPackets * 4, st));
    // the vector paths: whole 4-frame groups inside a packet, aligned loads at every group
    const FloatLayout layout =
        a.frameSize % 4 == 0 ? pcm_in_layout(a.in, CB, a.channels, a.channelStride, a.frameStride) : kFloatGeneral;
    const uint64_t bpp = ((uint64_t)a.frameSize + 1023) / 1024;
    const uint64_t blocks = (uint64_t)a.numPackets * bpp;
    const dim3 grid((uint32_t)(blocks < (1u << 22) ? blocks : (1u << 22)));
    switch (depth) {
    case 16: return launch_container<16>(a, dither, layout, grid, bpp, st);
    case 20: return launch_container<20>(a, dither, layout, grid, bpp, st);
    case 24: return launch_container<24>(a, dither, layout, grid, bpp, st);
    default: return launch_container<32>(a, dither, layout, grid, bpp, st);
    }
}

}  // namespace alacdev
