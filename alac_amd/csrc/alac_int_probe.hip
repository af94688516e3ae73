// alac_int_probe.hip — alac_hip_int_probe: one streaming pass over integer PCM that finds, per segment of frames, what names
// the smallest lossless bit depth (the rule of include/alac_hip.h: need(s) from the sample's trailing zeros, the containers
// out of range, the pad bits under a left-justified sample, the peak) and whether the channels are identical.  Reads what
// k_pcm_requantize (alac_pcm_in.hip) reads, through its loaders and in its layouts, with the geometry and the segment
// handling of k_float_probe (alac_float_probe.hip), and writes only the reports.
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_pcm_load.hpp"
#include "alac_probe_seg.hpp"

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

__device__ __forceinline__ void int_probe_merge(IntAcc &a, const IntAcc &b)
{
    a.bits |= b.bits;
    a.peak = b.peak > a.peak ? b.peak : a.peak;
    a.pad |= b.pad;
    a.oor += b.oor;
    a.diff += b.diff;
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

// a wave's accumulators reduced over its 64 lanes (every lane gets the result)
__device__ __forceinline__ void int_probe_wave_reduce(const IntAcc &a, uint32_t &bits, uint32_t &peak, uint32_t &pad,
                                                      uint64_t &oor, uint64_t &diff)
{
    bits = a.bits, peak = a.peak, pad = a.pad, oor = a.oor, diff = a.diff;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t p2 = __shfl_xor(peak, m);
        bits |= __shfl_xor(bits, m);
        pad |= __shfl_xor(pad, m);
        peak = p2 > peak ? p2 : peak;
        oor += __shfl_xor((unsigned long long)oor, m);
        diff += __shfl_xor((unsigned long long)diff, m);
    }
}

// the containers of one frame's channels (v[c], c < n) into the frame's accumulator
template <int N>
__device__ __forceinline__ void int_probe_frame(const int32_t (&v)[N], const IntProbeRule &R, IntAcc &fa)
{
    const int32_t s0 = int_probe_sample(v[0], R, fa);
#pragma unroll
    for (int c = 1; c < N; c++) fa.diff |= int_probe_sample(v[c], R, fa) != s0;
}

// The geometry of k_float_probe.  One lane: the 4 consecutive frames [f0, f0 + 4) of every channel, f0 a multiple of 4; a
// wave: 256 consecutive frames; a block: 1 024; a grid-stride loop over the blocks that cover [lo & ~3, hi).  CB: the
// container's bytes.  CH: 1 or 2 (the vector layouts of pcm_in_layout) or 0 (kFloatGeneral, a.channels at run time, one
// load per sample).  A group that lies in [lo, hi) whole is read with load_run in the vector layouts; frames outside
// [lo, hi) are never read.  The segment handling is k_float_probe's too: a wave whose in-range frames all lie in the segment
// of its first one adds them to per-lane accumulators that live across the loop and go out — one wave reduction, one atomic
// per field that moves — when the wave's segment changes, and at the end of the kernel once per block where its waves ended
// in the same segment; a wave that straddles a boundary takes the per-lane path.
// The per-lane counts are 32-bit: a lane sees at most 32 samples per 1 024 * gridDim.x frames of the call.
template <int CB, int CH, int LAYOUT>
__global__ __launch_bounds__(256) void k_int_probe(IntProbeArgs a)
{
    __shared__ uint32_t shSeg[4], shBits[4], shPeak[4], shPad[4];
    __shared__ uint64_t shOor[4], shDiff[4];
    const IntProbeRule R = int_probe_rule<CB>(a);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t g0 = a.lo & ~3ull;
    const uint64_t totalBlocks = (a.hi - g0 + 1023) / 1024;
    const uint32_t C = CH ? CH : a.channels;
    const IntAcc none = {0, 0, 0, 0, 0};
    IntAcc acc = none;
    uint32_t accSeg = kProbeNoSegment;
    for (uint64_t vb = blockIdx.x; vb < totalBlocks; vb += gridDim.x) {
        const uint64_t fw = g0 + vb * 1024 + wave * 256u;  // the wave's first frame
        const uint64_t wa = fw > a.lo ? fw : a.lo;          // ... inside [lo, hi)
        if (wa >= a.hi) continue;                           // (wave-uniform)
        const uint64_t f0 = fw + lane * 4u;
        // frames [f0 + b0, f0 + b1) of the lane's group lie in [lo, hi)
        const uint32_t b0 = f0 >= a.lo ? 0u : (a.lo - f0 < 4 ? (uint32_t)(a.lo - f0) : 4u);
        const uint32_t b1 = f0 >= a.hi ? 0u : (a.hi - f0 < 4 ? (uint32_t)(a.hi - f0) : 4u);
        IntAcc fa[4] = {none, none, none, none};  // per frame of the group
        if (LAYOUT != kFloatGeneral && b0 == 0 && b1 == 4) {
            if constexpr (LAYOUT == kFloatPlanar) {
                int32_t v[CH ? CH : 1][4];
#pragma unroll
                for (int c = 0; c < CH; c++) load_run<CB, 4>((const uint8_t *)a.in + (c * a.channelStride + f0) * CB, v[c]);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    int32_t fr[CH ? CH : 1];
#pragma unroll
                    for (int c = 0; c < CH; c++) fr[c] = v[c][k];
                    int_probe_frame(fr, R, fa[k]);
                }
            } else if constexpr (LAYOUT == kFloatInterleaved) {
                int32_t e[4 * (CH ? CH : 1)];
                load_run<CB, 4 * (CH ? CH : 1)>((const uint8_t *)a.in + f0 * (CH * CB), e);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    int32_t fr[CH ? CH : 1];
#pragma unroll
                    for (int c = 0; c < CH; c++) fr[c] = e[k * CH + c];
                    int_probe_frame(fr, R, fa[k]);
                }
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (k >= b0 && k < b1) {
                    const uint64_t at = (f0 + k) * a.frameStride;
                    const int32_t s0 = int_probe_sample(load_container<CB>(a.in, at), R, fa[k]);
                    for (uint32_t c = 1; c < C; c++)
                        fa[k].diff |= int_probe_sample(load_container<CB>(a.in, c * a.channelStride + at), R, fa[k]) != s0;
                }
        }
        // the wave's segment: that of its first frame in range
        // (without a table the one segment ends at hi, where b1 ends the lane's frames: every lane is inside.  Written so
        // that the segment's end is loaded only where there is a table: as `end = hi, or the table's entry` the compiler
        // selected between two addresses, one of them a copy of hi in scratch memory, which the kernel otherwise never uses)
        uint32_t s = 0;
        bool inside = true;
        if (a.segFirst) {
            s = probe_segment(a.segFirst, a.numSegments, wa);
            inside = b0 >= b1 || f0 + b1 <= a.segFirst[s + 1];
        }
        if (__ballot(inside) == ~0ull) {
            if (s != accSeg) {
                if (accSeg != kProbeNoSegment) {
                    uint32_t bits, peak, pad;
                    uint64_t oor, diff;
                    int_probe_wave_reduce(acc, bits, peak, pad, oor, diff);
                    if (lane == 0) int_probe_add(a.reports + 8ull * accSeg, R.S, bits, peak, pad, oor, diff);
                }
                acc = none;
                accSeg = s;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) int_probe_merge(acc, fa[k]);
        } else if (b0 < b1) {
            // mixed wave: the lane's frames one by one, consecutive frames of one segment added together
            uint32_t ls = probe_segment(a.segFirst, a.numSegments, f0 + b0);
            IntAcc run = none;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                if (k < b0 || k >= b1) continue;
                if (f0 + k >= a.segFirst[ls + 1]) {
                    int_probe_add(a.reports + 8ull * ls, R.S, run.bits, run.peak, run.pad, run.oor, run.diff);
                    run = none;
                    ls = probe_segment(a.segFirst, a.numSegments, f0 + k);
                }
                int_probe_merge(run, fa[k]);
            }
            int_probe_add(a.reports + 8ull * ls, R.S, run.bits, run.peak, run.pad, run.oor, run.diff);
        }
    }
    // what the waves still hold: one set of atomics per run of waves that ended in the same segment
    {
        uint32_t bits, peak, pad;
        uint64_t oor, diff;
        int_probe_wave_reduce(acc, bits, peak, pad, oor, diff);
        if (lane == 0)
            shSeg[wave] = accSeg, shBits[wave] = bits, shPeak[wave] = peak, shPad[wave] = pad, shOor[wave] = oor, shDiff[wave] = diff;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t seg = kProbeNoSegment, bits = 0, peak = 0, pad = 0;
        uint64_t oor = 0, diff = 0;
        for (int w = 0; w < 4; w++) {
            if (shSeg[w] != seg) {
                if (seg != kProbeNoSegment) int_probe_add(a.reports + 8ull * seg, R.S, bits, peak, pad, oor, diff);
                seg = shSeg[w], bits = 0, peak = 0, pad = 0, oor = 0, diff = 0;
            }
            bits |= shBits[w];
            pad |= shPad[w];
            peak = shPeak[w] > peak ? shPeak[w] : peak;
            oor += shOor[w];
            diff += shDiff[w];
        }
        if (seg != kProbeNoSegment) int_probe_add(a.reports + 8ull * seg, R.S, bits, peak, pad, oor, diff);
    }
}

template <int CB>
static hipError_t launch_layout(const IntProbeArgs &a, FloatLayout layout, dim3 grid, hipStream_t st)
{
    if (layout == kFloatGeneral) return launch_kernel(k_int_probe<CB, 0, kFloatGeneral>, grid, dim3(256), st, a);
    if (a.channels == 1) return launch_kernel(k_int_probe<CB, 1, kFloatPlanar>, grid, dim3(256), st, a);
    if (layout == kFloatInterleaved) return launch_kernel(k_int_probe<CB, 2, kFloatInterleaved>, grid, dim3(256), st, a);
    if constexpr (CB != 3)  // pcm_in_layout names no planar layout of two rows of packed 3-byte containers
        return launch_kernel(k_int_probe<CB, 2, kFloatPlanar>, grid, dim3(256), st, a);
    return hipErrorInvalidValue;
}

hipError_t launch_int_probe(const IntProbeArgs &a, hipStream_t st)
{
    const uint32_t S = a.srcBits, CB = a.containerBytes;
    if (a.numSegments == 0 || (S != 16 && S != 20 && S != 24 && S != 32) || CB < 2 || CB > 4 || S > 8 * CB ||
        a.channels < 1 || a.channels > kMaxChannels)
        return hipErrorInvalidValue;
    ALAC_TRY(hipMemsetAsync(a.reports, 0, (uint64_t)a.numSegments * 32, st));
    if (a.hi <= a.lo) return hipSuccess;
    const FloatLayout layout = pcm_in_layout(a.in, CB, a.channels, a.channelStride, a.frameStride);
    const uint64_t blocks = (a.hi - (a.lo & ~3ull) + 1023) / 1024;
    const dim3 grid((uint32_t)(blocks < kProbeMaxBlocks ? blocks : kProbeMaxBlocks));
    switch (CB) {
    case 2: return launch_layout<2>(a, layout, grid, st);
    case 3: return launch_layout<3>(a, layout, grid, st);
    default: return launch_layout<4>(a, layout, grid, st);
    }
}

}  // namespace alacdev
