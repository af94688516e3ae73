// alac_int_probe.hip — alac_hip_int_probe: one streaming pass over integer PCM that finds, per segment of frames, what names
// the smallest lossless bit depth (the rule of include/alac_hip.h: need(s) from the sample's trailing zeros, the containers
// out of range, the pad bits under a left-justified sample, the peak) and whether the channels are identical.  Reads what
// k_pcm_requantize (alac_pcm_in.hip) reads, through its loaders and in its layouts, on the walk k_float_probe
// (alac_float_probe.hip) takes (probe_walk, alac_probe_walk.hpp), and writes only the reports.
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_pcm_load.hpp"
#include "alac_probe_walk.hpp"

namespace alacdev {

// what a call's source comes to, the same for every container (scalars)
struct IntProbeRule {
    uint32_t rsh, padMask;  // left-justified: P = 8 * container bytes - S and 2^P - 1; else 0 and 0
    int32_t lo, hi;         // [-2^(S-1), 2^(S-1) - 1]: what a right-justified container is saturated to
    uint32_t S;
};

template <int CB>
__device__ __forceinline__ IntProbeRule int_probe_rule(const IntProbeArgs &a)
{
    IntProbeRule r;
    r.S = a.srcBits;
    r.rsh = a.leftJustified ? 8u * CB - r.S : 0u;
    r.padMask = (1u << r.rsh) - 1u;
    r.hi = (int32_t)(0x7fffffffu >> (32u - r.S));
    r.lo = ~r.hi;
    return r;
}

// what a set of samples adds to a report.  bits: the OR of the samples; ctz(a | b) = min(ctz(a), ctz(b)), so the largest
// need(s) = S - ctz(s) of the set is S - ctz(bits), one OR per sample in place of a count and a maximum
struct IntAcc {
    uint32_t bits, peak, pad, oor, diff;
};

// one container -> its sample; a zero container moves nothing, so a frame that is not read counts as 0
__device__ __forceinline__ int32_t int_probe_sample(int32_t v, const IntProbeRule &R, IntAcc &a)
{
    const int32_t s0 = v >> R.rsh;
    const int32_t s = min(max(s0, R.lo), R.hi);  // a left-justified sample lies inside: only right-justified ones saturate
    const uint32_t mag = s < 0 ? 0u - (uint32_t)s : (uint32_t)s;
    a.bits |= (uint32_t)s;
    a.peak = mag > a.peak ? mag : a.peak;
    a.pad |= (uint32_t)v & R.padMask;
    a.oor += s != s0;
    return s;
}

// adds to one report (8 words: alac_hip_int_report); a field that would not move is not sent
__device__ __forceinline__ void int_probe_add(uint32_t *report, uint32_t S, uint32_t bits, uint32_t peak, uint32_t pad,
                                              uint64_t oor, uint64_t diff)
{
    if (oor) atomicAdd((unsigned long long *)report, (unsigned long long)oor);
    if (diff) atomicAdd((unsigned long long *)(report + 2), (unsigned long long)diff);
    if (bits) atomicMax(report + 4, S - (uint32_t)(__ffs((int)bits) - 1));  // ctz = ffs - 1
    if (peak) atomicMax(report + 5, peak);
    if (pad) atomicOr(report + 6, pad);
}

// the containers of one frame's channels (v[c], c < n) into the frame's accumulator
template <int N>
__device__ __forceinline__ void int_probe_frame(const int32_t (&v)[N], const IntProbeRule &R, IntAcc &fa)
{
    const int32_t s0 = int_probe_sample(v[0], R, fa);
#pragma unroll
    for (int c = 1; c < N; c++) fa.diff |= int_probe_sample(v[c], R, fa) != s0;
}

// the integer rule of probe_walk (alac_probe_walk.hpp).  CB: the container's bytes; the containers come in through the loaders
// of alac_pcm_load.hpp
template <int CB>
struct IntProbe {
    using Acc = IntAcc;
    struct Sum {
        uint32_t bits, peak, pad;
        uint64_t oor, diff;
    };
    struct Shared {
        uint64_t oor[4], diff[4];
        uint32_t bits[4], peak[4], pad[4];
    };
    IntProbeRule R;

    static __device__ __forceinline__ void put(Shared &sh, uint32_t w, const Sum &s)
    {
        sh.bits[w] = s.bits, sh.peak[w] = s.peak, sh.pad[w] = s.pad, sh.oor[w] = s.oor, sh.diff[w] = s.diff;
    }
    static __device__ __forceinline__ Sum get(const Shared &sh, int w)
    {
        return {sh.bits[w], sh.peak[w], sh.pad[w], sh.oor[w], sh.diff[w]};
    }

    template <int CH, int LAYOUT>
    __device__ __forceinline__ void load_group(const IntProbeArgs &a, uint64_t f0, Acc (&fa)[4]) const
    {
        int32_t v[CH][4];
        if constexpr (LAYOUT == kFloatPlanar) {
#pragma unroll
            for (int c = 0; c < CH; c++) load_run<CB, 4>((const uint8_t *)a.in + (c * a.channelStride + f0) * CB, v[c]);
        } else {
            int32_t e[4 * CH];
            load_run<CB, 4 * CH>((const uint8_t *)a.in + f0 * (CH * CB), e);
#pragma unroll
            for (int j = 0; j < 4 * CH; j++) v[j % CH][j / CH] = e[j];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int32_t fr[CH];
#pragma unroll
            for (int c = 0; c < CH; c++) fr[c] = v[c][k];
            int_probe_frame(fr, R, fa[k]);
        }
    }
    __device__ __forceinline__ void load_frame(const IntProbeArgs &a, uint64_t f, uint32_t C, Acc &fa) const
    {
        const uint64_t at = f * a.frameStride;
        const int32_t s0 = int_probe_sample(load_container<CB>(a.in, at), R, fa);
        for (uint32_t c = 1; c < C; c++)
            fa.diff |= int_probe_sample(load_container<CB>(a.in, c * a.channelStride + at), R, fa) != s0;
    }
    template <typename T>
    static __device__ __forceinline__ void merge(T &a, const T &b)
    {
        a.bits |= b.bits;
        a.peak = b.peak > a.peak ? b.peak : a.peak;
        a.pad |= b.pad;
        a.oor += b.oor;
        a.diff += b.diff;
    }
    static __device__ __forceinline__ Sum reduce(const Acc &a)
    {
        Sum s = {a.bits, a.peak, a.pad, a.oor, a.diff};
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t p2 = __shfl_xor(s.peak, m);
            s.bits |= __shfl_xor(s.bits, m);
            s.pad |= __shfl_xor(s.pad, m);
            s.peak = p2 > s.peak ? p2 : s.peak;
            s.oor += __shfl_xor((unsigned long long)s.oor, m);
            s.diff += __shfl_xor((unsigned long long)s.diff, m);
        }
        return s;
    }
    template <typename T>
    __device__ __forceinline__ void add(uint32_t *report, const T &v) const
    {
        int_probe_add(report, R.S, v.bits, v.peak, v.pad, v.oor, v.diff);
    }
};

template <int CB, int CH, int LAYOUT>
__global__ __launch_bounds__(256) void k_int_probe(IntProbeArgs a)
{
    probe_walk<CH, LAYOUT>(IntProbe<CB>{int_probe_rule<CB>(a)}, a);
}

template <int CB>
static hipError_t launch_layout(const IntProbeArgs &a, hipStream_t st)
{
    const FloatLayout layout = pcm_in_layout(a.in, CB, a.channels, a.channelStride, a.frameStride);
    return launch_probe_walk(a, layout, st, [&](auto ch, auto lay, dim3 grid) {
        constexpr int CH = decltype(ch)::value, LAYOUT = decltype(lay)::value;
        // pcm_in_layout names no planar layout of two rows of packed 3-byte containers
        if constexpr (CB == 3 && CH == 2 && LAYOUT == kFloatPlanar) return hipErrorInvalidValue;
        else return launch_kernel(k_int_probe<CB, CH, LAYOUT>, grid, dim3(256), st, a);
    });
}

hipError_t launch_int_probe(const IntProbeArgs &a, hipStream_t st)
{
    const uint32_t S = a.srcBits, CB = a.containerBytes;
    if (a.numSegments == 0 || (S != 16 && S != 20 && S != 24 && S != 32) || CB < 2 || CB > 4 || S > 8 * CB ||
        a.channels < 1 || a.channels > kMaxChannels)
        return hipErrorInvalidValue;
    switch (CB) {
    case 2: return launch_layout<2>(a, st);
    case 3: return launch_layout<3>(a, st);
    default: return launch_layout<4>(a, st);
    }
}

}  // namespace alacdev
