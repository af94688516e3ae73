// alac_float_probe.hip — alac_hip_float_probe: one streaming pass over float32 PCM that finds, per segment of frames, what
// names the smallest lossless bit depth (the rule of include/alac_hip.h: need(x) from the bit pattern, range and NaN counts,
// the peak).  Reads what k_float_to_pcm (alac_float_in.hip) reads, in its three layouts, and writes only the reports.
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_probe_walk.hpp"

namespace alacdev {

// what a set of samples adds to a report: max need, max |x| as bits, samples out of range, NaNs
struct ProbeAcc {
    uint32_t need, peak, over, nan;
};

// one sample by its bit pattern: integer work only.  +-0.0 moves nothing, so a frame that is not read counts as 0.0f.
__device__ __forceinline__ void probe_sample(uint32_t u, ProbeAcc &a)
{
    const uint32_t mag = u & 0x7fffffffu;
    const bool isNan = mag > 0x7f800000u;
    a.nan += isNan;
    a.peak = isNan || mag < a.peak ? a.peak : mag;
    a.over += !isNan && (mag > 0x3f800000u || u == 0x3f800000u);  // x >= 1.0 or x < -1.0
    const uint32_t E = mag >> 23, M = mag & 0x7fffffu;
    const uint32_t sig = E ? M | 0x800000u : M;
    const int32_t lsb = E ? (int32_t)E - 150 : -149;
    const int32_t n = 1 - (lsb + __ffs((int)sig) - 1);  // ctz = ffs - 1 (sig != 0)
    const uint32_t need = sig != 0 && E != 255 && n > 0 ? (uint32_t)n : 0u;
    a.need = need > a.need ? need : a.need;
}

// adds to one report (8 words: alac_hip_float_report); a field that would not move is not sent
__device__ __forceinline__ void probe_add(uint32_t *report, uint32_t need, uint32_t peak, uint64_t over, uint64_t nan)
{
    if (over) atomicAdd((unsigned long long *)report, (unsigned long long)over);
    if (nan) atomicAdd((unsigned long long *)(report + 2), (unsigned long long)nan);
    if (need) atomicMax(report + 4, need);
    if (peak) atomicMax(report + 5, peak);
}

// the float32 rule of probe_walk (alac_probe_walk.hpp)
struct FloatProbe {
    using Acc = ProbeAcc;
    struct Sum {
        uint32_t need, peak;
        uint64_t over, nan;
    };
    struct Shared {
        uint32_t need[4], peak[4];
        uint64_t over[4], nan[4];
    };
    static __device__ __forceinline__ void put(Shared &sh, uint32_t w, const Sum &s)
    {
        sh.need[w] = s.need, sh.peak[w] = s.peak, sh.over[w] = s.over, sh.nan[w] = s.nan;
    }
    static __device__ __forceinline__ Sum get(const Shared &sh, int w) { return {sh.need[w], sh.peak[w], sh.over[w], sh.nan[w]}; }

    template <int CH, int LAYOUT>
    __device__ __forceinline__ void load_group(const FloatProbeArgs &a, uint64_t f0, Acc (&fa)[4]) const
    {
        if constexpr (LAYOUT == kFloatPlanar) {
#pragma unroll
            for (int c = 0; c < CH; c++) {
                const uint4 v = *(const uint4 *)(a.in + c * a.channelStride + f0);
                probe_sample(v.x, fa[0]), probe_sample(v.y, fa[1]), probe_sample(v.z, fa[2]), probe_sample(v.w, fa[3]);
            }
        } else if constexpr (LAYOUT == kFloatInterleaved) {
            const uint4 v = *(const uint4 *)(a.in + f0 * 2), w = *(const uint4 *)(a.in + f0 * 2 + 4);
            probe_sample(v.x, fa[0]), probe_sample(v.y, fa[0]), probe_sample(v.z, fa[1]), probe_sample(v.w, fa[1]);
            probe_sample(w.x, fa[2]), probe_sample(w.y, fa[2]), probe_sample(w.z, fa[3]), probe_sample(w.w, fa[3]);
        }
    }
    __device__ __forceinline__ void load_frame(const FloatProbeArgs &a, uint64_t f, uint32_t C, Acc &fa) const
    {
        for (uint32_t c = 0; c < C; c++) probe_sample(__float_as_uint(a.in[c * a.channelStride + f * a.frameStride]), fa);
    }
    template <typename T>
    static __device__ __forceinline__ void merge(T &a, const T &b)
    {
        a.need = b.need > a.need ? b.need : a.need;
        a.peak = b.peak > a.peak ? b.peak : a.peak;
        a.over += b.over;
        a.nan += b.nan;
    }
    static __device__ __forceinline__ Sum reduce(const Acc &a)
    {
        Sum s = {a.need, a.peak, a.over, a.nan};
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t n2 = __shfl_xor(s.need, m), p2 = __shfl_xor(s.peak, m);
            s.need = n2 > s.need ? n2 : s.need;
            s.peak = p2 > s.peak ? p2 : s.peak;
            s.over += __shfl_xor((unsigned long long)s.over, m);
            s.nan += __shfl_xor((unsigned long long)s.nan, m);
        }
        return s;
    }
    template <typename T>
    __device__ __forceinline__ void add(uint32_t *report, const T &v) const
    {
        probe_add(report, v.need, v.peak, v.over, v.nan);
    }
};

template <int CH, int LAYOUT>
__global__ __launch_bounds__(256) void k_float_probe(FloatProbeArgs a)
{
    probe_walk<CH, LAYOUT>(FloatProbe(), a);
}

hipError_t launch_float_probe(const FloatProbeArgs &a, hipStream_t st)
{
    if (a.numSegments == 0) return hipErrorInvalidValue;
    const FloatLayout layout = pcm_in_layout(a.in, 4, a.channels, a.channelStride, a.frameStride);
    return launch_probe_walk(a, layout, st, [&](auto ch, auto lay, dim3 grid) {
        return launch_kernel(k_float_probe<decltype(ch)::value, decltype(lay)::value>, grid, dim3(256), st, a);
    });
}

}  // namespace alacdev
