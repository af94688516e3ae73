// alac_probe_seg.hpp — what the two probe passes (alac_float_probe.hip, alac_int_probe.hip) share: the segment of a frame,
// the "no segment yet" mark of a wave's accumulators and the cap of the grid.
#pragma once
#include "alac_dev.hpp"

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

}  // namespace alacdev
