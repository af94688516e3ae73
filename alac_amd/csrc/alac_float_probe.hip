// alac_float_probe.hip — alac_hip_float_probe: one streaming pass over float32 PCM that finds, per segment of frames, what
// names the smallest lossless bit depth (the rule of include/alac_hip.h: need(x) from the bit pattern, range and NaN counts,
// the peak).  Reads what k_float_to_pcm (alac_float_in.hip) reads, in its three layouts, and writes only the reports.
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_probe_seg.hpp"

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

__device__ __forceinline__ void probe_merge(ProbeAcc &a, const ProbeAcc &b)
{
    a.need = b.need > a.need ? b.need : a.need;
    a.peak = b.peak > a.peak ? b.peak : a.peak;
    a.over += b.over;
    a.nan += b.nan;
}

// adds to one report (8 words: alac_hip_float_report); a field that would not move is not sent
__device__ __forceinline__ void probe_add(uint32_t *report, uint32_t need, uint32_t peak, uint64_t over, uint64_t nan)
{
    if (over) atomicAdd((unsigned long long *)report, (unsigned long long)over);
    if (nan) atomicAdd((unsigned long long *)(report + 2), (unsigned long long)nan);
    if (need) atomicMax(report + 4, need);
    if (peak) atomicMax(report + 5, peak);
}

// a wave's accumulators reduced over its 64 lanes (every lane gets the result)
__device__ __forceinline__ void probe_wave_reduce(const ProbeAcc &a, uint32_t &need, uint32_t &peak, uint64_t &over,
                                                  uint64_t &nan)
{
    need = a.need, peak = a.peak, over = a.over, nan = a.nan;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t n2 = __shfl_xor(need, m), p2 = __shfl_xor(peak, m);
        need = n2 > need ? n2 : need;
        peak = p2 > peak ? p2 : peak;
        over += __shfl_xor((unsigned long long)over, m);
        nan += __shfl_xor((unsigned long long)nan, m);
    }
}

// One lane: the 4 consecutive frames [f0, f0 + 4) of every channel, f0 a multiple of 4; a wave: 256 consecutive frames; a
// block: 1 024; a grid-stride loop over the blocks that cover [lo & ~3, hi).  CH: 1 or 2 (the vector layouts: aligned
// strides and base, the host checks) or 0 (kFloatGeneral, a.channels at run time).  A group that lies in [lo, hi) whole is
// read with 16-byte loads in the vector layouts; frames outside [lo, hi) are never read.
// A wave whose in-range frames all lie in the segment of its first one (one ballot) adds them to per-lane accumulators that
// live across the loop; they go out — one wave reduction, one atomic per field that moves — when the wave's segment
// changes, and at the end of the kernel once per block where its waves ended in the same segment.  A wave that straddles a
// boundary takes the per-lane path: every lane finds the segments of its own frames and adds to their reports itself.
// The per-lane counts are 32-bit: a lane sees at most 32 samples per 1 024 * gridDim.x frames of the call.
template <int CH, int LAYOUT>
__global__ __launch_bounds__(256) void k_float_probe(FloatProbeArgs a)
{
    __shared__ uint32_t shSeg[4], shNeed[4], shPeak[4];
    __shared__ uint64_t shOver[4], shNan[4];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t g0 = a.lo & ~3ull;
    const uint64_t totalBlocks = (a.hi - g0 + 1023) / 1024;
    const uint32_t C = CH ? CH : a.channels;
    ProbeAcc acc = {0, 0, 0, 0};
    uint32_t accSeg = kProbeNoSegment;
    for (uint64_t vb = blockIdx.x; vb < totalBlocks; vb += gridDim.x) {
        const uint64_t fw = g0 + vb * 1024 + wave * 256u;  // the wave's first frame
        const uint64_t wa = fw > a.lo ? fw : a.lo;          // ... inside [lo, hi)
        if (wa >= a.hi) continue;                           // (wave-uniform)
        const uint64_t f0 = fw + lane * 4u;
        // frames [f0 + b0, f0 + b1) of the lane's group lie in [lo, hi)
        const uint32_t b0 = f0 >= a.lo ? 0u : (a.lo - f0 < 4 ? (uint32_t)(a.lo - f0) : 4u);
        const uint32_t b1 = f0 >= a.hi ? 0u : (a.hi - f0 < 4 ? (uint32_t)(a.hi - f0) : 4u);
        ProbeAcc fa[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};  // per frame of the group
        if (LAYOUT != kFloatGeneral && b0 == 0 && b1 == 4) {
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
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (k >= b0 && k < b1)
                    for (uint32_t c = 0; c < C; c++)
                        probe_sample(__float_as_uint(a.in[c * a.channelStride + (f0 + k) * a.frameStride]), fa[k]);
        }
        // the wave's segment: that of its first frame in range
        uint32_t s = 0;
        uint64_t end = a.hi;
        if (a.segFirst) {
            s = probe_segment(a.segFirst, a.numSegments, wa);
            end = a.segFirst[s + 1];
        }
        const bool inside = b0 >= b1 || f0 + b1 <= end;
        if (__ballot(inside) == ~0ull) {
            if (s != accSeg) {
                if (accSeg != kProbeNoSegment) {
                    uint32_t need, peak;
                    uint64_t over, nan;
                    probe_wave_reduce(acc, need, peak, over, nan);
                    if (lane == 0) probe_add(a.reports + 8ull * accSeg, need, peak, over, nan);
                }
                acc = {0, 0, 0, 0};
                accSeg = s;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) probe_merge(acc, fa[k]);
        } else if (b0 < b1) {
            // mixed wave: the lane's frames one by one, consecutive frames of one segment added together
            uint32_t ls = probe_segment(a.segFirst, a.numSegments, f0 + b0);
            ProbeAcc run = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                if (k < b0 || k >= b1) continue;
                if (f0 + k >= a.segFirst[ls + 1]) {
                    probe_add(a.reports + 8ull * ls, run.need, run.peak, run.over, run.nan);
                    run = {0, 0, 0, 0};
                    ls = probe_segment(a.segFirst, a.numSegments, f0 + k);
                }
                probe_merge(run, fa[k]);
            }
            probe_add(a.reports + 8ull * ls, run.need, run.peak, run.over, run.nan);
        }
    }
    // what the waves still hold: one set of atomics per run of waves that ended in the same segment
    {
        uint32_t need, peak;
        uint64_t over, nan;
        probe_wave_reduce(acc, need, peak, over, nan);
        if (lane == 0) shSeg[wave] = accSeg, shNeed[wave] = need, shPeak[wave] = peak, shOver[wave] = over, shNan[wave] = nan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t seg = kProbeNoSegment, need = 0, peak = 0;
        uint64_t over = 0, nan = 0;
        for (int w = 0; w < 4; w++) {
            if (shSeg[w] != seg) {
                if (seg != kProbeNoSegment) probe_add(a.reports + 8ull * seg, need, peak, over, nan);
                seg = shSeg[w], need = 0, peak = 0, over = 0, nan = 0;
            }
            need = shNeed[w] > need ? shNeed[w] : need;
            peak = shPeak[w] > peak ? shPeak[w] : peak;
            over += shOver[w];
            nan += shNan[w];
        }
        if (seg != kProbeNoSegment) probe_add(a.reports + 8ull * seg, need, peak, over, nan);
    }
}

hipError_t launch_float_probe(const FloatProbeArgs &a, hipStream_t st)
{
    if (a.numSegments == 0) return hipErrorInvalidValue;
    ALAC_TRY(hipMemsetAsync(a.reports, 0, (uint64_t)a.numSegments * 32, st));
    if (a.hi <= a.lo) return hipSuccess;
    const FloatLayout layout = float_layout(a.in, a.channels, a.channelStride, a.frameStride);
    const uint64_t blocks = (a.hi - (a.lo & ~3ull) + 1023) / 1024;
    const dim3 grid((uint32_t)(blocks < kProbeMaxBlocks ? blocks : kProbeMaxBlocks));
    if (layout == kFloatGeneral) return launch_kernel(k_float_probe<0, kFloatGeneral>, grid, dim3(256), st, a);
    if (a.channels == 1) return launch_kernel(k_float_probe<1, kFloatPlanar>, grid, dim3(256), st, a);
    if (layout == kFloatPlanar) return launch_kernel(k_float_probe<2, kFloatPlanar>, grid, dim3(256), st, a);
    return launch_kernel(k_float_probe<2, kFloatInterleaved>, grid, dim3(256), st, a);
}

}  // namespace alacdev
