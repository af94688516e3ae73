// alac_true_peak.hip — alac_hip_true_peak_int / alac_hip_true_peak_float: the true peak of ITU-R BS.1770-4 annex 2 of PCM where
// it lies, per segment of frames and per channel, and the host-only filter query.  The rule is in include/alac_hip.h.
//
// The interpolator is an FIR, so there is one pass and nothing to carry: a segment is cut into runs of true_peak_run(F) frames,
// one lane each, and a lane reads the K - 1 frames in front of its run again as history (zeros at a segment's start, never
// loads) — the run of a segment's last frame also flushes the K - 1 outputs behind it.  A lane's stream of frames goes by in
// slices of 16: the slice's samples stand behind the K - 1 of history in one register array, and every output of the slice is
// a fully unrolled chain of K fused multiply-adds per phase over it.  Maxima only, so the result does not depend on who
// computed what: lane to wave to block, then one 64-bit atomicMax per block, segment and channel on the bits of the
// non-negative double.  Sources and staged loads: alac_loud_source.hpp, as k_loud_pass.  DESIGN.md section 25.
#include "alac_hip.h"
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_loud_source.hpp"
#include "alac_pcm_load.hpp"
#include "alac_probe_walk.hpp"

#include <cmath>
#include <cstdlib>

namespace alacdev {

void true_peak_coefs(uint32_t F, double (&coef)[kTruePeakMaxCoefs])
{
    const double pi = 3.14159265358979323846;
    const uint32_t K = true_peak_taps(F);
    for (uint32_t i = 0; i < kTruePeakMaxCoefs; i++) coef[i] = 0.0;
    for (uint32_t j = 0; j <= 48 && F > 1; j++) {
        const uint32_t p = j % F, k = j / F;
        if (p == 0) continue;  // phase 0 is the tap 1.0 at the centre: the sample itself, not filtered
        const double m = (double)j - 24.0, arg = m * pi / (double)F;
        coef[(p - 1) * K + k] = std::sin(arg) / arg * (0.5 * (1.0 - std::cos(2.0 * pi * (double)j / 48.0)));
    }
}

__device__ __forceinline__ void true_peak_add(uint64_t *word, double m)
{
    const unsigned long long bits = (unsigned long long)__double_as_longlong(m);  // m >= +0.0: the bits order as m does
    if (bits) atomicMax((unsigned long long *)word, bits);
}

// One lane: one run of a.run frames — all CH channels of it in a vector layout (CH 1 or 2), one channel of it in the general
// layout (CH 0: blockIdx.y is the channel, so that a block reduces one channel).
// The lane's stream: `halo` frames of history (K - 1, or 0 at the segment's start: positions [0, outBegin), read but neither
// counted nor measured), its own frames ([outBegin, inEnd)), and behind a segment's last frame K - 1 zeros ([inEnd, outEnd)).
// Interleaved stereo and mono: the loads are staged through LDS (LoudStage), a barrier on both sides of every slice's loads;
// every thread of the block runs every slice.  Planar stereo and the general layout, and every layout under
// ALAC_HIP_TRUE_PEAK_DIRECT=1: each lane loads its own containers.  The same operations on the same values both ways.
// F 1: nothing is filtered, K - 1 = 0, the maximum of |x| alone.
template <typename Src, int CH, int LAYOUT, int F>
__global__ __launch_bounds__(256) void k_true_peak(TruePeakArgs a)
{
    constexpr int NC = CH ? CH : 1;
    constexpr int CB = Src::kBytes;
    constexpr bool STAGED = LAYOUT == kFloatInterleaved || (LAYOUT == kFloatPlanar && CH == 1);
    constexpr int FB = NC * CB;
    constexpr int K = F == 4 ? 12 : F == 2 ? 24 : 1, H = K - 1, P = F - 1, SL = 16;
    static_assert(SL == (int)LoudStage<FB>::kFrames, "a slice is what LoudStage stages");
    const Src src(a);
    const uint32_t C = CH ? CH : a.channels;
    const uint32_t c0 = CH ? 0u : blockIdx.y;
    const uint64_t g = blockIdx.x * 256ull + threadIdx.x;
    const bool active = g < a.totalChunks;
    uint32_t s = 0, halo = 0, frames = 0;
    uint64_t f0 = 0, segFirst = 0, segEnd = 0;
    bool last = false;
    if (active) {
        s = probe_segment(a.chunkBase, a.numSegments, g);
        const uint64_t j = g - a.chunkBase[s];
        segFirst = a.segFirst[s], segEnd = a.segFirst[s + 1];
        f0 = segFirst + j * a.run;
        const uint64_t f1 = f0 + a.run < segEnd ? f0 + a.run : segEnd;
        frames = (uint32_t)(f1 - f0);
        halo = j ? (uint32_t)H : 0u;  // a.run >= K - 1: the history lies in the run before, inside the segment
        last = f1 == segEnd;
    }
    const uint32_t outBegin = halo, inEnd = halo + frames, outEnd = inEnd + (last ? (uint32_t)H : 0u);
    // the slices every thread of the block runs: those of a whole run, and where a segment ends in the block those of its tail
    const uint32_t slices = (H + a.run + (__syncthreads_or(last) ? H : 0) + SL - 1) / SL;

    double xx[NC][H + SL], m[NC];
    uint32_t peakWord[NC], nonfinite = 0;  // per channel: the sample peak's word
#pragma unroll
    for (int c = 0; c < NC; c++) {
        m[c] = 0.0, peakWord[c] = 0;
#pragma unroll
        for (int j = 0; j < H; j++) xx[c][j] = 0.0;
    }
    // sample i of the slice at `base`: xx, and where it is a frame of the run itself the sample peak's word and the count.
    // (The masks are factors 1.0 or 0.0 where that is one instruction for a select's two: v is finite, so v * 0.0 is a zero)
    auto take = [&](int c, int i, uint32_t base, uint32_t raw) {
        const uint32_t pos = base + i;
        uint32_t pk = 0, nf = 0;
        const double v = src.value(raw, pk, nf);
        const bool in = pos < inEnd, own = in && pos >= outBegin;
        xx[c][H + i] = v * (in ? 1.0 : 0.0);
        pk = own ? pk : 0u;
        peakWord[c] = pk > peakWord[c] ? pk : peakWord[c];
        nonfinite += own ? nf : 0u;
    };
    // the slice's outputs, and the window moves on
    auto filter = [&](uint32_t base) {
        if constexpr (P > 0) {
#pragma unroll
            for (int i = 0; i < SL; i++) {
                const uint32_t pos = base + i;
                const double valid = pos >= outBegin && pos < outEnd ? 1.0 : 0.0;
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    double best = 0.0;
#pragma unroll
                    for (int p = 0; p < P; p++) {
                        double acc = 0.0;
#pragma unroll
                        for (int k = 0; k < K; k++) acc = fma(a.coef[p * K + k], xx[c][H + i - k], acc);
                        best = fmax(best, fabs(acc));
                    }
                    m[c] = fmax(m[c], best * valid);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int j = 0; j < H; j++) xx[c][j] = xx[c][j + SL];
    };

    bool direct = true;
    if constexpr (STAGED) {
        direct = a.direct != 0;  // (uniform)
        if (!direct) {
            __shared__ LoudStage<FB> S;
            const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
            const uint64_t before = (f0 - halo - segFirst) * FB, behind = (segEnd - (f0 + frames)) * FB;
            const uint64_t first = (uint64_t)(uintptr_t)a.in + (f0 - halo) * FB;
            S.first[w][lane] = first;
            S.total[w][lane] = inEnd * FB;
            S.slack[w][lane] = (uint32_t)(before < 15 ? before : 15) | (uint32_t)(behind < 15 ? behind : 15) << 8;
            const uint8_t *row = S.rows[w] + lane * LoudStage<FB>::kRow + (first & 15);
#pragma unroll 1
            for (uint32_t t = 0; t < slices; t++) {
                __syncthreads();  // the descriptors are written; the rows of the slice before are read
                loud_stage_slice(S, w, lane, t);
                __syncthreads();
#pragma unroll
                for (int i = 0; i < SL; i++)
#pragma unroll
                    for (int c = 0; c < NC; c++) take(c, i, t * SL, (uint32_t)load_container<CB>(row, i * NC + c));
                filter(t * SL);
            }
        }
    }
    if (direct) {
#pragma unroll 1
        for (uint32_t t = 0; t * SL < outEnd; t++) {
#pragma unroll
            for (int i = 0; i < SL; i++) {
                const uint64_t f = f0 - halo + t * SL + i;
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    uint32_t raw = 0;
                    if (t * SL + i < inEnd) raw = (uint32_t)load_container<CB>(a.in, (c0 + c) * a.channelStride + f * a.frameStride);
                    take(c, i, t * SL, raw);
                }
            }
            filter(t * SL);
        }
    }

    // the sample peak: per channel into its maximum (the value the report's peak has where the channel holds it), over the
    // channels the report's word
    uint32_t peak = 0;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        m[c] = fmax(m[c], src.peak_value(peakWord[c]));
        peak = peakWord[c] > peak ? peakWord[c] : peak;
    }
    // lane -> wave -> block, where they lie in one segment
    auto wave_max = [&]() {
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) {
            const uint32_t p2 = __shfl_xor(peak, x);
            peak = p2 > peak ? p2 : peak;
            nonfinite += __shfl_xor(nonfinite, x);
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const double m2 = __shfl_xor(m[c], x);
                m[c] = m2 > m[c] ? m2 : m[c];
            }
        }
    };
    auto add = [&](uint32_t seg) {
        loud_add(a.reports + 8ull * seg, peak, nonfinite);
#pragma unroll
        for (int c = 0; c < NC; c++) true_peak_add(a.channelPeak + (uint64_t)seg * C + c0 + c, m[c]);
    };
    const uint32_t sb = probe_segment(a.chunkBase, a.numSegments, blockIdx.x * 256ull);  // the block's first run is active
    if (!__syncthreads_or(active && s != sb)) {
        __shared__ double shM[4][NC];
        __shared__ uint32_t shPeak[4], shCount[4];
        wave_max();
        if ((threadIdx.x & 63) == 0) {
            shPeak[threadIdx.x >> 6] = peak, shCount[threadIdx.x >> 6] = nonfinite;
#pragma unroll
            for (int c = 0; c < NC; c++) shM[threadIdx.x >> 6][c] = m[c];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; w++) {
                peak = shPeak[w] > peak ? shPeak[w] : peak;
                nonfinite += shCount[w];
#pragma unroll
                for (int c = 0; c < NC; c++) m[c] = shM[w][c] > m[c] ? shM[w][c] : m[c];
            }
            add(sb);
        }
    } else {
        const uint32_t first = __shfl(s, 0);  // lane 0 is active wherever a lane of the wave is
        if (__ballot(active && s != first) == 0) {
            wave_max();
            if ((threadIdx.x & 63) == 0 && active) add(first);
        } else if (active) {
            add(s);
        }
    }
}

// per segment: the maximum over the channels, the peak's word as a double, and the words that are not collected
template <typename Src>
__global__ __launch_bounds__(256) void k_true_peak_finish(TruePeakArgs a)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.numSegments) return;
    const Src src(a);
    uint32_t *d = a.reports + 8ull * s;
    const double peak = src.peak_value(d[2]);
    double tp = 0.0;
    for (uint32_t c = 0; c < a.channels; c++) {
        const double v = __longlong_as_double((long long)a.channelPeak[(uint64_t)s * a.channels + c]);
        tp = v > tp ? v : tp;
    }
    *(double *)d = tp;
    *(double *)(d + 2) = peak;
    d[6] = 0, d[7] = 0;
}

template <typename Src>
static hipError_t launch_source(const TruePeakArgs &a, hipStream_t st)
{
    constexpr int CB = Src::kBytes;
    const uint32_t C = a.channels;
    ALAC_TRY(hipMemsetAsync(a.reports, 0, (uint64_t)a.numSegments * 32, st));
    ALAC_TRY(hipMemsetAsync(a.channelPeak, 0, (uint64_t)a.numSegments * C * 8, st));
    if (a.totalChunks) {
        const uint64_t blocks = (a.totalChunks + 255) / 256;
        if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
        const FloatLayout layout = pcm_in_layout(a.in, CB, C, a.channelStride, a.frameStride);
        auto pass = [&](auto factor) {
            return dispatch_layout(layout, C, [&](auto ch, auto lay) {
                constexpr int CH = decltype(ch)::value, LAYOUT = decltype(lay)::value, F = decltype(factor)::value;
                // pcm_in_layout names no planar layout of two rows of packed 3-byte containers
                if constexpr (CB == 3 && CH == 2 && LAYOUT == kFloatPlanar) return hipErrorInvalidValue;
                else
                    return launch_kernel(k_true_peak<Src, CH, LAYOUT, F>, dim3((uint32_t)blocks, CH ? 1u : C), dim3(256), st, a);
            });
        };
        switch (a.factor) {
        case 4: ALAC_TRY(pass(std::integral_constant<int, 4>())); break;
        case 2: ALAC_TRY(pass(std::integral_constant<int, 2>())); break;
        default: ALAC_TRY(pass(std::integral_constant<int, 1>())); break;
        }
    }
    return launch_kernel(k_true_peak_finish<Src>, dim3((a.numSegments + 255) / 256), dim3(256), st, a);
}

hipError_t launch_true_peak(const TruePeakArgs &args, hipStream_t st)
{
    TruePeakArgs a = args;
    const char *direct = getenv("ALAC_HIP_TRUE_PEAK_DIRECT");  // the measurement switch: no staging through LDS
    a.direct = direct && direct[0] == '1';
    const uint32_t S = a.srcBits, CB = a.containerBytes;
    if (a.numSegments == 0 || a.channels < 1 || a.channels > kMaxChannels || (a.factor != 4 && a.factor != 2 && a.factor != 1) ||
        a.run != true_peak_run(a.factor))
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

int32_t alac_hip_true_peak_filter(uint32_t sample_rate, uint32_t *out_factor, uint32_t *out_taps, double *out_coefs)
{
    if (!out_factor || !out_taps || !out_coefs || !loud_rate_ok(sample_rate)) return ALAC_HIP_ParamError;
    const uint32_t F = true_peak_factor(sample_rate), K = true_peak_taps(F);
    double c[kTruePeakMaxCoefs];
    true_peak_coefs(F, c);
    *out_factor = F, *out_taps = K;
    for (uint32_t i = 0; i < (F - 1) * K; i++) out_coefs[i] = c[i];
    return ALAC_HIP_noErr;
}
