// alac_resample.hip — alac_hip_resample_int / alac_hip_resample_float: sample-rate conversion of PCM where it lies, per segment
// of frames, and the host-only plan, filter and frame-count queries.  The rule is in include/alac_hip.h.
//
// A polyphase windowed-sinc FIR in double over the sample value of alac_loud_source.hpp, as k_true_peak, but the outputs are
// kept: planar float32, which is what alac_hip_encode_float takes.  A segment's output frames are cut into tiles of
// resample_tile() frames, one block each.  The block loads the input span its tile needs once into LDS as doubles, zeros
// where the span reaches over an end of the segment (so nothing outside a segment is read and the taps need no bounds), and
// a lane then computes output frames: all channels of a frame in the vector layouts, so a coefficient is loaded once per
// frame, and two frames at a time, so that 2 or 4 chains of fused multiply-adds are independent.  The coefficients come from
// the table in the workspace, two taps per 16-byte load; it lies there as [K/2][L][2], so that the 64 phases a wave needs at
// one step lie in L * 16 bytes (20 lines of 128 bytes at L = 160) and not in 64 rows.  Every output has one owner and one
// order of summation.  The peak is a maximum over the bits of |float32 written|, lane to wave to block to one atomicMax.
// DESIGN.md section 27.
#include "alac_hip.h"
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_loud_source.hpp"
#include "alac_pcm_load.hpp"
#include "alac_probe_walk.hpp"

#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <vector>

namespace alacdev {

ResamplePlan resample_plan(uint32_t inRate, uint32_t outRate)
{
    ResamplePlan p = {0, 0, 0, false};
    if (!loud_rate_ok(inRate) || !loud_rate_ok(outRate) || inRate == outRate) return p;
    const uint32_t g = std::gcd(inRate, outRate);
    p.L = outRate / g, p.M = inRate / g;
    if (p.L > 640 || p.M > 640) return p;
    const uint32_t big = p.L > p.M ? p.L : p.M;
    p.K = 2 * ((40 * big + p.L - 1) / p.L);
    p.ok = true;
    return p;
}

// I0 by its power series, sum_j ((x / 2)^j / j!)^2: every term positive, so nothing cancels
static double bessel_i0(double x)
{
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int j = 1; j < 500; j++) {
        term *= q / ((double)j * (double)j);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

static void resample_fill(const ResamplePlan &p, double *out)
{
    const double pi = 3.14159265358979323846, beta = 10.0;
    const double c = (double)(p.L < p.M ? p.L : p.M) / (double)p.M, i0b = bessel_i0(beta);
    for (uint32_t ph = 0; ph < p.L; ph++) {
        for (uint32_t k = 0; k < p.K; k++) {
            const double t = (double)ph / (double)p.L + (double)k - (double)(p.K / 2);
            const double u = c * t, r = 2.0 * t / (double)p.K, w = 1.0 - r * r;
            const double sinc = u == 0.0 ? 1.0 : std::sin(pi * u) / (pi * u);
            out[(size_t)ph * p.K + k] = c * sinc * bessel_i0(beta * std::sqrt(w > 0.0 ? w : 0.0)) / i0b;
        }
    }
}

const double *resample_coefs(const ResamplePlan &p)
{
    static std::mutex mu;
    static std::map<uint64_t, std::unique_ptr<std::vector<double>>> kept;
    std::lock_guard<std::mutex> lock(mu);
    std::unique_ptr<std::vector<double>> &v = kept[(uint64_t)p.L << 32 | p.M];
    if (!v) {
        // phase-major [L][K], what alac_hip_resample_filter hands out, then the kernels' arrangement [K/2][L][2]
        const size_t n = (size_t)p.L * p.K;
        v.reset(new std::vector<double>(2 * n));
        double *h = v->data(), *t = h + n;
        resample_fill(p, h);
        for (uint32_t ph = 0; ph < p.L; ph++)
            for (uint32_t k = 0; k < p.K; k++) t[((size_t)(k / 2) * p.L + ph) * 2 + (k & 1)] = h[(size_t)ph * p.K + k];
    }
    return v->data();
}

// One block: one tile of a.tile output frames of one segment — all CH channels of them in a vector layout (CH 1 or 2), one
// channel in the general layout (CH 0: blockIdx.y is the channel).
// Output m of the segment: n0 = m M div L, p = m M mod L, y = sum_k h_p[k] x[n0 + K/2 - k].  The tile's outputs [m0, m0 + T)
// need the frames [lo, hi] = [n0(m0) - K/2 + 1, n0(m0 + T - 1) + K/2] of the segment, at most a.span of them: LDS position i
// holds frame lo + i, 0.0 where that is not a frame of the segment.  The non-finite samples are counted where a frame is the
// tile's own: frames [ceil(m0 M / L), ceil((m0 + T) M / L)) — the segment's first tile from 0, its last one up to N — which
// lie inside the span because K/2 >= 40 M / L.
template <typename Src, int CH, int LAYOUT>
__global__ __launch_bounds__(256) void k_resample(ResampleArgs a)
{
    constexpr int NC = CH ? CH : 1;
    constexpr int CB = Src::kBytes;
    extern __shared__ double x[];  // [span][NC]
    __shared__ uint32_t shPeak[4], shCount[4];
    const Src src(a);
    const uint32_t c0 = CH ? 0u : blockIdx.y;
    const uint32_t tid = threadIdx.x;
    const uint64_t L = a.L, M = a.M;
    const uint32_t K = a.K, half = K / 2;

    const uint32_t s = probe_segment(a.tileBase, a.numSegments, blockIdx.x);
    const uint64_t segFirst = a.segFirst[s], N = a.segFirst[s + 1] - segFirst;
    const uint64_t outFirst = a.outFirst[s], outN = a.outFirst[s + 1] - outFirst;
    const uint64_t m0 = (blockIdx.x - a.tileBase[s]) * a.tile;
    const uint32_t T = (uint32_t)(outN - m0 < a.tile ? outN - m0 : a.tile);  // >= 1: the tile exists
    const int64_t lo = (int64_t)(m0 * M / L) - (int64_t)half + 1;
    const uint32_t count = (uint32_t)((int64_t)((m0 + T - 1) * M / L) + half - lo + 1);  // <= a.span
    const uint64_t ownLo = m0 ? (m0 * M + L - 1) / L : 0;
    const uint64_t ownHi = m0 + T == outN ? N : ((m0 + T) * M + L - 1) / L;

    uint32_t nonfinite = 0, peak = 0;
    for (uint32_t i = tid; i < count; i += 256) {
        const int64_t n = lo + (int64_t)i;
        double v[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) v[c] = 0.0;
        if (n >= 0 && (uint64_t)n < N) {
            const uint64_t f = segFirst + (uint64_t)n;
            uint32_t raw[NC];
            if constexpr (LAYOUT == kFloatInterleaved && CB == 2) {  // (pcm_in_layout: the base is 8-byte aligned)
                const uint32_t w = ((const uint32_t *)a.in)[f];
                raw[0] = (uint32_t)(int32_t)(int16_t)w, raw[1] = (uint32_t)((int32_t)w >> 16);
            } else if constexpr (LAYOUT == kFloatInterleaved && CB == 4) {  // (... 16-byte aligned)
                const uint2 w = ((const uint2 *)a.in)[f];
                raw[0] = w.x, raw[1] = w.y;
            } else {
#pragma unroll
                for (int c = 0; c < NC; c++)
                    raw[c] = (uint32_t)load_container<CB>(a.in, (c0 + c) * a.channelStride + f * a.frameStride);
            }
            const bool own = (uint64_t)n >= ownLo && (uint64_t)n < ownHi;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                uint32_t pk = 0, nf = 0;
                v[c] = src.value(raw[c], pk, nf);
                nonfinite += own ? nf : 0u;
            }
        }
#pragma unroll
        for (int c = 0; c < NC; c++) x[(size_t)i * NC + c] = v[c];
    }
    __syncthreads();

    float *out = a.out + c0 * a.outChannelStride + outFirst + m0;
    for (uint32_t o = tid; o < T; o += 512) {
        // two outputs of the lane, 256 apart; where the second one lies behind the tile it repeats the first and is not stored
        const bool two = o + 256 < T;
        const uint32_t oo[2] = {o, two ? o + 256 : o};
        const double2 *h[2];
        const double *xp[2];
        double acc[2][NC];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const uint64_t mm = (m0 + oo[q]) * M, n0 = mm / L, p = mm - n0 * L;
            h[q] = (const double2 *)a.coef + p;  // taps 2 kk and 2 kk + 1 of phase p at [kk][p]
            xp[q] = x + (size_t)((int64_t)n0 + half - lo) * NC;  // x[n0 + K/2] of the segment; tap k lies k frames below
#pragma unroll
            for (int c = 0; c < NC; c++) acc[q][c] = 0.0;
        }
#pragma unroll 2
        for (uint32_t kk = 0; kk < half; kk++) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const double2 hh = h[q][(size_t)kk * L];
                const double *x0 = xp[q] - (size_t)(2 * kk) * NC, *x1 = x0 - NC;
                if constexpr (NC == 2) {
                    const double2 v0 = *(const double2 *)x0, v1 = *(const double2 *)x1;
                    acc[q][0] = fma(hh.x, v0.x, acc[q][0]), acc[q][1] = fma(hh.x, v0.y, acc[q][1]);
                    acc[q][0] = fma(hh.y, v1.x, acc[q][0]), acc[q][1] = fma(hh.y, v1.y, acc[q][1]);
                } else {
                    acc[q][0] = fma(hh.x, x0[0], acc[q][0]);
                    acc[q][0] = fma(hh.y, x1[0], acc[q][0]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 2; q++) {
            if (q == 1 && !two) break;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const float y = (float)acc[q][c];
                out[c * a.outChannelStride + oo[q]] = y;
                const uint32_t mag = __float_as_uint(y) & 0x7fffffffu;
                peak = mag > peak ? mag : peak;
            }
        }
    }

    // lane -> wave -> block -> the segment's report
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t p2 = __shfl_xor(peak, d);
        peak = p2 > peak ? p2 : peak;
        nonfinite += __shfl_xor(nonfinite, d);
    }
    if ((tid & 63) == 0) shPeak[tid >> 6] = peak, shCount[tid >> 6] = nonfinite;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) {
            peak = shPeak[w] > peak ? shPeak[w] : peak;
            nonfinite += shCount[w];
        }
        loud_add(a.reports + 8ull * s, peak, nonfinite);
    }
}

// per segment: the words the pass collected (2: the peak's float bits, 4-5: the count) become the report
__global__ __launch_bounds__(256) void k_resample_finish(ResampleArgs a)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.numSegments) return;
    uint32_t *d = a.reports + 8ull * s;
    const double peak = (double)__uint_as_float(d[2]);
    const uint64_t nonfinite = *(const uint64_t *)(d + 4);
    *(uint64_t *)d = a.outFirst[s];
    *(uint64_t *)(d + 2) = a.outFirst[s + 1] - a.outFirst[s];
    *(double *)(d + 4) = peak;
    *(uint64_t *)(d + 6) = nonfinite;
}

template <typename Src>
static hipError_t launch_source(const ResampleArgs &a, hipStream_t st)
{
    constexpr int CB = Src::kBytes;
    const uint32_t C = a.channels;
    ALAC_TRY(hipMemsetAsync(a.reports, 0, (uint64_t)a.numSegments * 32, st));
    if (a.totalTiles) {
        if (a.totalTiles > 0x7fffffffull) return hipErrorInvalidValue;
        const FloatLayout layout = pcm_in_layout(a.in, CB, C, a.channelStride, a.frameStride);
        ALAC_TRY(dispatch_layout(layout, C, [&](auto ch, auto lay) {
            constexpr int CH = decltype(ch)::value, LAYOUT = decltype(lay)::value;
            // pcm_in_layout names no planar layout of two rows of packed 3-byte containers
            if constexpr (CB == 3 && CH == 2 && LAYOUT == kFloatPlanar) return hipErrorInvalidValue;
            else
                return launch_kernel_lds(k_resample<Src, CH, LAYOUT>, dim3((uint32_t)a.totalTiles, CH ? 1u : C), dim3(256),
                                         (size_t)a.span * (CH ? CH : 1) * 8, st, a);
        }));
    }
    return launch_kernel(k_resample_finish, dim3((a.numSegments + 255) / 256), dim3(256), st, a);
}

hipError_t launch_resample(const ResampleArgs &a, hipStream_t st)
{
    const uint32_t S = a.srcBits, CB = a.containerBytes;
    if (a.numSegments == 0 || a.channels < 1 || a.channels > kMaxChannels || a.L < 1 || a.M < 1 || a.K < 2 || (a.K & 1) ||
        a.tile < 1 || (uint64_t)a.span * 16 > kResampleLdsBytes || ((uintptr_t)a.coef & 15))
        return hipErrorInvalidValue;
    if (CB == 0) return launch_source<LoudFloat>(a, st);
    if ((S != 16 && S != 20 && S != 24 && S != 32) || CB < 2 || CB > 4 || S > 8 * CB) return hipErrorInvalidValue;
    switch (CB) {
    case 2: return launch_source<LoudInt<2>>(a, st);
    case 3: return launch_source<LoudInt<3>>(a, st);
    default: return launch_source<LoudInt<4>>(a, st);
    }
}

}  // namespace alacdev

// ---- host only ----------------------------------------------------------------------------------------------------------------
using namespace alacdev;

int32_t alac_hip_resample_filter(uint32_t in_rate, uint32_t out_rate, uint32_t *out_L, uint32_t *out_M, uint32_t *out_K,
                                 double *out_coefs)
{
    const ResamplePlan p = resample_plan(in_rate, out_rate);
    if (!out_L || !out_M || !out_K || !p.ok) return ALAC_HIP_ParamError;
    *out_L = p.L, *out_M = p.M, *out_K = p.K;
    if (out_coefs) {
        const double *c = resample_coefs(p);
        for (size_t i = 0; i < (size_t)p.L * p.K; i++) out_coefs[i] = c[i];
    }
    return ALAC_HIP_noErr;
}

uint64_t alac_hip_resample_frames(uint32_t in_rate, uint32_t out_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                  uint32_t num_segments, uint64_t *h_out_first)
{
    const ResamplePlan p = resample_plan(in_rate, out_rate);
    if (!p.ok || num_segments == 0 || (!h_seg_first_frame && num_segments != 1) || total_frames > UINT64_MAX / 1024) return 0;
    if (h_seg_first_frame) {
        for (uint32_t s = 0; s < num_segments; s++)
            if (h_seg_first_frame[s] > h_seg_first_frame[s + 1]) return 0;
        if (h_seg_first_frame[num_segments] > total_frames) return 0;
    }
    uint64_t total = 0;
    for (uint32_t s = 0; s < num_segments; s++) {
        if (h_out_first) h_out_first[s] = total;
        total += resample_out_frames(p, h_seg_first_frame ? h_seg_first_frame[s + 1] - h_seg_first_frame[s] : total_frames);
    }
    if (h_out_first) h_out_first[num_segments] = total;
    return total;
}
