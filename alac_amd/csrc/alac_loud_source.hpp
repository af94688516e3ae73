// alac_loud_source.hpp — what the measuring passes over PCM (k_loud_pass, alac_loudness.hip, and k_true_peak,
// alac_true_peak.hip) share: how a raw container becomes the sample value x of the rule in include/alac_hip.h, with the peak's
// word and the non-finite count, and how a wave whose lanes sit a whole run of frames apart stages its loads through LDS.
// DESIGN.md sections 24 and 25.
#pragma once
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_pcm_load.hpp"

namespace alacdev {

// ---- what a source format adds: a raw container -> x, the peak's word and the non-finite count ----
// the peak's word orders as |x| does: |s| of an integer sample, the bit pattern of |f| of a finite float
// (Args: LoudArgs or TruePeakArgs, for srcBits and leftJustified)
template <int CB>
struct LoudInt {
    static constexpr int kBytes = CB;
    uint32_t rsh;
    int32_t lo, hi;
    double scale;  // 2^-(S-1)
    template <typename Args>
    __device__ __forceinline__ explicit LoudInt(const Args &a)
    {
        const uint32_t S = a.srcBits;
        rsh = a.leftJustified ? 8u * CB - S : 0u;
        hi = (int32_t)(0x7fffffffu >> (32u - S));
        lo = ~hi;
        scale = __hiloint2double((int)((1023u - (S - 1u)) << 20), 0);
    }
    __device__ __forceinline__ double value(uint32_t raw, uint32_t &peak, uint32_t &nonfinite) const
    {
        const int32_t s = min(max((int32_t)raw >> rsh, lo), hi);
        const uint32_t mag = s < 0 ? 0u - (uint32_t)s : (uint32_t)s;
        peak = mag > peak ? mag : peak;
        return (double)s * scale;  // exact: |s| <= 2^31
    }
    __device__ __forceinline__ double peak_value(uint32_t word) const { return (double)word * scale; }
};

struct LoudFloat {
    static constexpr int kBytes = 4;
    template <typename Args>
    __device__ __forceinline__ explicit LoudFloat(const Args &)
    {
    }
    __device__ __forceinline__ double value(uint32_t raw, uint32_t &peak, uint32_t &nonfinite) const
    {
        const uint32_t mag = raw & 0x7fffffffu;
        const bool finite = mag < 0x7f800000u;
        nonfinite += !finite;
        peak = finite && mag > peak ? mag : peak;
        return finite ? (double)__uint_as_float(raw) : 0.0;
    }
    __device__ __forceinline__ double peak_value(uint32_t word) const { return (double)__uint_as_float(word); }
};

// adds to one report (8 words: alac_hip_loudness_report or alac_hip_true_peak_report; word 2 collects the peak's word, words
// 4-5 the count)
__device__ __forceinline__ void loud_add(uint32_t *report, uint32_t peak, uint32_t nonfinite)
{
    if (peak) atomicMax(report + 2, peak);
    if (nonfinite) atomicAdd((unsigned long long *)(report + 4), (unsigned long long)nonfinite);
}

// The staged loads of a pass (frame-contiguous vector layouts: interleaved stereo and mono, FB bytes per frame).  The lanes of
// a wave sit a run of frames apart, so the wave takes its 64 runs in time slices of kFrames frames: the 64 pieces of a slice
// (kRun bytes each) are loaded kPieces 16-byte pieces per run — consecutive lanes take consecutive pieces, at 16-byte aligned
// addresses from the run's first byte rounded down — into the wave's 64 rows of LDS, and lane k then walks row k.  A row is
// kRow bytes: its pieces and one pad word, an odd count of words, so that the 64 lanes' reads fall into different banks.
template <int FB>
struct LoudStage {
    static constexpr uint32_t kFrames = 16, kRun = kFrames * FB, kPieces = kRun / 16 + 1, kRow = 16 * kPieces + 4;
    uint8_t rows[4][64 * kRow];  // per wave of the block
    uint64_t first[4][64];       // per lane: the address of its run's first byte
    uint32_t total[4][64];       // ... the run's bytes (0: nothing to load)
    uint32_t slack[4][64];       // ... the bytes of the segment in front of the run (low byte) and behind it, each up to 15
};

// slice t of the wave's runs into its rows.  A piece that lies inside the segment is one aligned 16-byte load; a piece that
// reaches over an end of the segment is loaded byte by byte, its bytes inside the run only: nothing outside the segment is read
template <int FB>
__device__ __forceinline__ void loud_stage_slice(LoudStage<FB> &S, uint32_t w, uint32_t lane, uint32_t t)
{
    using St = LoudStage<FB>;
    for (uint32_t q = lane; q < 64 * St::kPieces; q += 64) {
        const uint32_t k = q / St::kPieces, i = q % St::kPieces;
        const uint32_t tot = S.total[w][k], done = t * St::kRun;
        if (done >= tot) continue;
        const uint32_t n = tot - done < St::kRun ? tot - done : St::kRun;
        const uint64_t b = S.first[w][k] + done, e = b + n;
        const uint64_t p = (b & ~15ull) + 16 * i;
        if (p >= e) continue;
        const uint32_t sl = S.slack[w][k], behind = (sl >> 8) + (tot - done - n);
        const uint64_t lo = b - (t ? 15u : (sl & 255u)), hi = e + (behind < 15 ? behind : 15u);
        uint8_t *dst = S.rows[w] + k * St::kRow + 16 * i;
        if (p >= lo && p + 16 <= hi) {
            const uint4 v = *(const uint4 *)p;
            uint32_t *d = (uint32_t *)dst;
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else {
            for (uint32_t x = 0; x < 16; x++)
                if (p + x >= b && p + x < e) dst[x] = *(const uint8_t *)(p + x);
        }
    }
}

}  // namespace alacdev
