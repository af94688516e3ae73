// alac_probe_walk.hpp — the walk of the two probe passes (k_float_probe, alac_float_probe.hip, and k_int_probe,
// alac_int_probe.hip): the geometry over [lo, hi), the segment of a frame, the accumulators a wave keeps per segment and how
// they reach the reports.  What a source format adds is its rule (what an accumulator holds and how samples move it), its
// kernel and its launcher.  DESIGN.md section 20.
#pragma once
#include "alac_dev.hpp"
#include "alac_kernels.hpp"

namespace alacdev {

// the segment of frame f, first[0] <= f < first[n]: the largest s with first[s] <= f (empty segments in front of it are
// passed over, and first[s + 1] > f)
__device__ __forceinline__ uint32_t probe_segment(const uint64_t *first, uint32_t n, uint64_t f)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= f) lo = mid;
        else hi = mid;
    }
    return lo;
}

constexpr uint32_t kProbeNoSegment = 0xffffffffu;

// blocks of a launch: few enough that the closing atomics of a one-segment call (two words of one report) stay a small
// part of the pass.  Not tuned, and a value to revisit: 1 024 blocks are 4 waves per SIMD, which streams 4.1 GB from HBM
// faster than k_float_to_pcm does but has too little in flight for a pass that lies in the Infinity Cache (328 MB: 88 us
// against 75 us); 2 048 (8 waves per SIMD, what the registers allow) is the value to try.  The
// tests' PASS constant (tests/test_gpu_float_probe.py, tests/test_gpu_int_probe.py) is 1 024 times this.
constexpr uint32_t kProbeMaxBlocks = 1024;

// One lane: the 4 consecutive frames [f0, f0 + 4) of every channel, f0 a multiple of 4; a wave: 256 consecutive frames; a
// block: 1 024; a grid-stride loop over the blocks that cover [lo & ~3, hi).  CH: 1 or 2 (the vector layouts of
// pcm_in_layout) or 0 (kFloatGeneral, a.channels at run time, one load per sample).  A group that lies in [lo, hi) whole is
// read with vector loads in the vector layouts; frames outside [lo, hi) are never read.
// A wave whose in-range frames all lie in the segment of its first one (one ballot) adds them to per-lane accumulators that
// live across the loop; they go out — one wave reduction, one atomic per field that moves — when the wave's segment
// changes, and at the end of the kernel once per block where its waves ended in the same segment.  A wave that straddles a
// boundary takes the per-lane path: every lane finds the segments of its own frames and adds to their reports itself.
// Rule: Acc, what a set of samples adds to a report, with 32-bit counts (a lane sees at most 32 samples per
// 1 024 * gridDim.x frames of the call), and Sum, the same with 64-bit counts, both zero as {}; load_group<CH, LAYOUT>(a, f0,
// fa), a whole group of a vector layout into its 4 per-frame accumulators; load_frame(a, f, C, fa), one frame; merge(x, y)
// of two Accs or two Sums; reduce(acc), the Sum over the wave's 64 lanes (every lane gets it); add(report, acc or sum);
// Shared, the four waves' Sums in LDS as one array per field, with put(sh, wave, sum) and get(sh, wave).
template <int CH, int LAYOUT, typename Rule, typename Args>
__device__ __forceinline__ void probe_walk(const Rule &R, const Args &a)
{
    using Acc = typename Rule::Acc;
    using Sum = typename Rule::Sum;
    __shared__ uint32_t shSeg[4];
    __shared__ typename Rule::Shared sh;  // the waves' sums, one array per field
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t g0 = a.lo & ~3ull;
    const uint64_t totalBlocks = (a.hi - g0 + 1023) / 1024;
    const uint32_t C = CH ? CH : a.channels;
    Acc acc = {};
    uint32_t accSeg = kProbeNoSegment;
    for (uint64_t vb = blockIdx.x; vb < totalBlocks; vb += gridDim.x) {
        const uint64_t fw = g0 + vb * 1024 + wave * 256u;  // the wave's first frame
        const uint64_t wa = fw > a.lo ? fw : a.lo;          // ... inside [lo, hi)
        if (wa >= a.hi) continue;                           // (wave-uniform)
        const uint64_t f0 = fw + lane * 4u;
        // frames [f0 + b0, f0 + b1) of the lane's group lie in [lo, hi)
        const uint32_t b0 = f0 >= a.lo ? 0u : (a.lo - f0 < 4 ? (uint32_t)(a.lo - f0) : 4u);
        const uint32_t b1 = f0 >= a.hi ? 0u : (a.hi - f0 < 4 ? (uint32_t)(a.hi - f0) : 4u);
        Acc fa[4] = {};  // per frame of the group
        if (LAYOUT != kFloatGeneral && b0 == 0 && b1 == 4) {
            if constexpr (LAYOUT != kFloatGeneral) R.template load_group<CH, LAYOUT>(a, f0, fa);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (k >= b0 && k < b1) R.load_frame(a, f0 + k, C, fa[k]);
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
                    const Sum sum = Rule::reduce(acc);
                    if (lane == 0) R.add(a.reports + 8ull * accSeg, sum);
                }
                acc = {};
                accSeg = s;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) Rule::merge(acc, fa[k]);
        } else if (b0 < b1) {
            // mixed wave: the lane's frames one by one, consecutive frames of one segment added together
            uint32_t ls = probe_segment(a.segFirst, a.numSegments, f0 + b0);
            Acc run = {};
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                if (k < b0 || k >= b1) continue;
                if (f0 + k >= a.segFirst[ls + 1]) {
                    R.add(a.reports + 8ull * ls, run);
                    run = {};
                    ls = probe_segment(a.segFirst, a.numSegments, f0 + k);
                }
                Rule::merge(run, fa[k]);
            }
            R.add(a.reports + 8ull * ls, run);
        }
    }
    // what the waves still hold: one set of atomics per run of waves that ended in the same segment
    const Sum held = Rule::reduce(acc);
    if (lane == 0) shSeg[wave] = accSeg, Rule::put(sh, wave, held);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t seg = kProbeNoSegment;
        Sum sum = {};
        for (int w = 0; w < 4; w++) {
            if (shSeg[w] != seg) {
                if (seg != kProbeNoSegment) R.add(a.reports + 8ull * seg, sum);
                seg = shSeg[w], sum = {};
            }
            Rule::merge(sum, Rule::get(sh, w));
        }
        if (seg != kProbeNoSegment) R.add(a.reports + 8ull * seg, sum);
    }
}

// the launch of a probe kernel: zeroes the reports, then (hi > lo) 1 024 frames per block, at most kProbeMaxBlocks blocks.
// launch(CH, LAYOUT, grid) starts the kernel of that pair.
template <typename Args, typename Launch>
inline hipError_t launch_probe_walk(const Args &a, FloatLayout layout, hipStream_t st, Launch launch)
{
    ALAC_TRY(hipMemsetAsync(a.reports, 0, (uint64_t)a.numSegments * 32, st));
    if (a.hi <= a.lo) return hipSuccess;
    const uint64_t blocks = (a.hi - (a.lo & ~3ull) + 1023) / 1024;
    const dim3 grid((uint32_t)(blocks < kProbeMaxBlocks ? blocks : kProbeMaxBlocks));
    return dispatch_layout(layout, a.channels, [&](auto ch, auto lay) { return launch(ch, lay, grid); });
}

}  // namespace alacdev
