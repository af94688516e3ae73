// alac_pcm_in.hip — integer PCM of any layout, container and depth -> the packed interleaved integer PCM alac_hip_encode
// reads (alac_hip_pcm_requantize, the conversion pass of alac_hip_encode_int).  One streaming pass in front of the unchanged
// encoder: take the sample out of its container, widen it or reduce it by the integer rule of include/alac_hip.h (round
// half to even, optionally TPDF dither from the generator of alac_float_rule.hpp), pack, count clips.
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_float_rule.hpp"
#include "alac_pcm_walk.hpp"
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

// the integer source of pcm_walk (alac_pcm_walk.hpp).  CB: the container's bytes
template <int DEPTH, int CB, bool DITHER>
struct IntSrc {
    using Elem = int32_t;
    static constexpr bool kDither = DITHER;
    const void *in;
    PcmInRule R;

    __device__ __forceinline__ int32_t load1(uint64_t idx) const { return load_container<CB>(in, idx); }
    template <int N>
    __device__ __forceinline__ void load_run(uint64_t idx, int32_t (&e)[N]) const
    {
        alacdev::load_run<CB, N>((const uint8_t *)in + idx * CB, e);
    }
    __device__ __forceinline__ void convert4(const int32_t (&v)[4], const bool (&live)[4], uint64_t t0, uint32_t c,
                                             const FloatDitherArgs &dz, int32_t (&s)[4], uint32_t &clips) const
    {
        int32_t z[4] = {0, 0, 0, 0};
        if constexpr (DITHER) dither4_k(t0, c, dz, z);
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) s[k] = requantize<DEPTH, DITHER>(v[k], live[k] ? z[k] : 0, R, clips);
    }
};

template <int DEPTH, int CB, int CH, int LAYOUT, bool DITHER>
__global__ __launch_bounds__(256) void k_pcm_requantize(PcmInArgs a, uint64_t blocksPerPacket, FloatDitherArgs dz)
{
    pcm_walk<DEPTH, CH, LAYOUT>(IntSrc<DEPTH, CB, DITHER>{a.in, pcm_in_rule<DEPTH, CB>(a)}, a, blocksPerPacket, dz);
}

template <int DEPTH, int CB, bool DITHER>
static hipError_t launch_layout(const PcmInArgs &a, const FloatDitherArgs &dz, hipStream_t st)
{
    const FloatLayout layout = pcm_in_layout(a.in, CB, a.channels, a.channelStride, a.frameStride);
    return launch_pcm_walk(a, layout, st, [&](auto ch, auto lay, dim3 grid, uint64_t bpp) {
        constexpr int CH = decltype(ch)::value, LAYOUT = decltype(lay)::value;
        // pcm_in_layout names no planar layout of two rows of packed 3-byte containers
        if constexpr (CB == 3 && CH == 2 && LAYOUT == kFloatPlanar) return hipErrorInvalidValue;
        else return launch_kernel(k_pcm_requantize<DEPTH, CB, CH, LAYOUT, DITHER>, grid, dim3(256), st, a, bpp, dz);
    });
}

// dither is a reduction's: 3- and 4-byte containers (a 2-byte one holds 16 bits, the smallest target)
template <int DEPTH>
static hipError_t launch_container(const PcmInArgs &a, const FloatDitherArgs *dz, hipStream_t st)
{
    const FloatDitherArgs none = {};
    if constexpr (DEPTH != 32) {
        if (dz && a.containerBytes == 3) return launch_layout<DEPTH, 3, true>(a, *dz, st);
        if (dz && a.containerBytes == 4) return launch_layout<DEPTH, 4, true>(a, *dz, st);
    }
    if (dz) return hipErrorInvalidValue;
    switch (a.containerBytes) {
    case 2: return launch_layout<DEPTH, 2, false>(a, none, st);
    case 3: return launch_layout<DEPTH, 3, false>(a, none, st);
    default: return launch_layout<DEPTH, 4, false>(a, none, st);
    }
}

hipError_t launch_pcm_requantize(uint32_t depth, const PcmInArgs &a, hipStream_t st, const FloatDitherArgs *dither)
{
    const uint32_t S = a.srcBits, CB = a.containerBytes;
    if ((depth != 16 && depth != 20 && depth != 24 && depth != 32) || (S != 16 && S != 20 && S != 24 && S != 32) ||
        CB < 2 || CB > 4 || S > 8 * CB || (dither && depth >= S))
        return hipErrorInvalidValue;
    switch (depth) {
    case 16: return launch_container<16>(a, dither, st);
    case 20: return launch_container<20>(a, dither, st);
    case 24: return launch_container<24>(a, dither, st);
    default: return launch_container<32>(a, dither, st);
    }
}

}  // namespace alacdev
