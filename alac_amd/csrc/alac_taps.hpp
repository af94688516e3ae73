// alac_taps.hpp — the 32-lane-half reductions of the tap-parallel predictor (one chain per half of a wave, lane k owns
// tap k): shared by the stage-level pc_block (alac_stage_taps.hip) and the LPC trial / final passes (alac_lpc.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "alac_dev.hpp"

namespace alacdev {
namespace taps {

constexpr int kQuadXor1 = 0xB1, kQuadXor2 = 0x4E, kRowHalfMirror = 0x141, kRowMirror = 0x140, kWaveShr1 = 0x138;

template <int CTRL>
__device__ __forceinline__ int32_t dpp0(int32_t v)  // out-of-range source lanes read 0
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}

// sum over the 32 lanes of each half, result in every lane
__device__ __forceinline__ int32_t half_sum(int32_t v)
{
    v += dpp0<kQuadXor1>(v);
    v += dpp0<kQuadXor2>(v);
    v += dpp0<kRowHalfMirror>(v);
    v += dpp0<kRowMirror>(v);
    v += __shfl_xor(v, 16, 32);
    return v;
}

// exclusive suffix sum over the 32 lanes of each half: S_k = sum_{i>k} w_i
__device__ __forceinline__ int32_t half_suffix_exclusive(int32_t w, int k)
{
    int32_t v = w;
    v += dpp0<0x101>(v);  // row_shl:1  lane k takes lane k+1 (0 past the end of the 16-lane row)
    v += dpp0<0x102>(v);  // row_shl:2
    v += dpp0<0x104>(v);
    v += dpp0<0x108>(v);
    const int32_t upper = __shfl(v, 16, 32);  // total of lanes 16..31 of this half
    v += k < 16 ? upper : 0;
    return v - w;
}

// One step of pc_block's general loop (dp_enc.c:341-387) for the chain of this half: lane k holds x = in[j - 1 - k] and,
// for k < na, coefficient a (adapted in place).  Returns the residual of `cur` = in[j], the same value in every lane of
// the half.  Called by whole halves only (the reductions read the other lanes of the half).
__device__ __forceinline__ int32_t taps_step(int32_t cur, int32_t x, int32_t &a, int32_t na, int k, uint32_t chanshift,
                                             uint32_t denshift)
{
    const bool tap = k < na;
    const int32_t denhalf = denshift ? (1 << (denshift - 1)) : 0;
    const int32_t round = (1 << denshift) - 1;
    const int32_t top = __shfl(x, na, 32);
    const int32_t dd = tap ? top - x : 0;
    const int32_t sum1 = half_sum(-a * dd);  // sum a_k (pin[-k] - top), int32 wrap as in the reference
    const int32_t del = sext(cur - top - ((sum1 + denhalf) >> denshift), chanshift);
    // coefficient walk (dp_enc.c:365-385)
    const int32_t sg = (del > 0) - (del < 0);
    const int32_t ab = dd < 0 ? -dd : dd;
    const int32_t t = (sg > 0 ? ab : ab + round) >> denshift;  // (sgn dd) >> ds resp. -((-sgn dd) >> ds)
    const int32_t S = half_suffix_exclusive((tap ? na - k : 0) * t, k);
    const int32_t adel = del < 0 ? -del : del;
    const int32_t sd = (dd > 0) - (dd < 0);
    if (tap && sg != 0 && adel > S) a = (int16_t)(a - sg * sd);
    return del;
}

// slide the window: lane k takes lane k-1's sample, lane 0 of each half the new one (whole wave)
__device__ __forceinline__ int32_t taps_slide(int32_t x, int32_t cur, int k)
{
    const int32_t shifted = __builtin_amdgcn_update_dpp(0, x, kWaveShr1, 0xf, 0xf, false);
    return k == 0 ? cur : shifted;
}

}  // namespace taps
}  // namespace alacdev
