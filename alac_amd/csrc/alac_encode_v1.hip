// alac_encode_v1.hip — dispatcher of the tap-parallel encode pipeline: the plan of a call (regime and shape), and the call
// into the per-depth launcher (alac_encode_v1_impl.hpp, instantiated in alac_encode_v1_d16/20/24/32.hip).
#include <cstdlib>
#include "alac_encode_v1_types.hpp"

namespace alacdev {

// init_coefs for every row of the working state (codec/ALACEncoder.cu:1524-1531)
__global__ void k_init_state(int16_t *state, uint32_t numSegments)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= numSegments * 64u) return;
    const uint32_t k = i & 15;
    state[i] = (int16_t)(k == 0 ? 1216 : k == 1 ? -928 : k == 2 ? -64 : 0);
}

__global__ void k_check_segments(const uint32_t *segFirst, uint32_t numSegments, uint32_t numPackets, uint32_t maxSeg, uint32_t *err,
                                 uint32_t *segBad)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= numSegments) return;
    const uint32_t a = segFirst[s], b = segFirst[s + 1];
    const bool bad = b < a || b > numPackets || b - a > maxSeg || (s == 0 && a != 0) || (s + 1 == numSegments && b != numPackets);
    if (bad && err) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (bad && segBad) *segBad = 1u;  // what the launches behind this one on the stream test (EncodeArgs::segBad)
}

hipError_t launch_check_segments(const uint32_t *segFirst, uint32_t numSegments, uint32_t numPackets, uint32_t maxSeg, uint32_t *err,
                                 uint32_t *segBad, hipStream_t st)
{
    if (segBad) ALAC_TRY(hipMemsetAsync(segBad, 0, 4, st));
    return launch_kernel(k_check_segments, dim3((numSegments + 255) / 256), dim3(256), st, segFirst, numSegments, numPackets, maxSeg,
                         err, segBad);
}

// chains beyond what one 2-lane predictor wave per SIMD holds (1024 SIMDs x 32 chains x 2): throughput regime
static bool v1_throughput_regime(uint32_t numSegments, uint32_t channels, const AlacOptions &opt)
{
    if (opt.thru >= 0) return opt.thru != 0;
    return (uint64_t)numSegments * (channels > 2 ? 2 : channels) > 65536;
}

// Four lanes per chain ("tiny") or two ("latency") below the throughput regime.  Every launch of these regimes is made of
// single-wave workers that want a SIMD to themselves (1024 SIMDs): five per 64 chains with four lanes per chain, three with two.
// The four-lane form has the shorter serial chain and wins while ITS workers fit (measured crossover 5 500-6 000 packets = 11 000-
// 12 000 chains, 16- and 24-bit); then the two-lane form while its workers fit (21 845 chains: at 10 000 packets 938 workers);
// behind that cliff — 10 500 -> 11 000 packets: 1.46 -> 2.26 ms, some SIMDs now carry two predictor waves — the four-lane form,
// already past its own cliff and flat, is faster again until ~17 000 packets (11 000 / 12 000 / 14 000 / 16 000 / 18 000 packets,
// four against two lanes: 1.81 / 2.26, 1.82 / 2.44, 2.23 / 2.49, 2.34 / 2.54, 2.64 / 2.61 ms; profiles/r04/encode_regime_sweep.log).
// Until round 4 the rule was "four lanes up to 4096 chains".  Mono streams (no mixRes search, whose five passes are where the
// four-lane form gains most) cross over earlier at both ends: 10 000 / 11 000 chains 0.93 / 0.99 against 1.07 / 1.00 ms, and
// 26 000 / 28 000 chains 1.55 / 1.77 against 1.97 / 1.78 — there the four-lane workers reach two per SIMD (26 214 chains).
static bool v1_narrow_regime(uint64_t chains, uint32_t channels, const AlacOptions &opt)
{
    if (opt.narrow >= 0) return opt.narrow != 0;
    const bool mono = channels == 1;
    if (chains <= (mono ? 10240u : 11264u)) return true;
    if (chains <= 21760) return false;  // 3 workers per 64 chains <= 1020
    return chains <= (mono ? 26112u : 34816u);
}

// Latency regime (about one wave per SIMD: up to ~2 x 1024 x 32 chains): idle lanes should not slow their wave down
// (V1Args::idleFast).  With many waves per SIMD the machine is throughput bound and the extra work of idle lanes costs more
// than the checked paths (measured: 125 000 packets 18.6 ms vs 20.3 ms).
V1Plan v1_plan(uint32_t channels, uint32_t numSegments, uint32_t maxSegPackets, uint32_t frameSize, const AlacOptions &opt)
{
    V1Plan P{};
    const uint32_t ch = channels > 2 ? 2 : channels;
    const uint64_t chains = (uint64_t)numSegments * ch;
    P.fast = ch == 2 && opt.fastMode != 0;  // SetFastMode: no search passes at all (mono has no fast form)
    if (opt.laneEncoder && !(channels == 2 && opt.fastMode))  // (the lane kernel has no search-free form: use_lane_encoder)
        P.shape = V1Shape::Lane;
    else if (v1_throughput_regime(numSegments, ch, opt))
        P.shape = V1Shape::Throughput;
    else if (!opt.fused)
        P.shape = V1Shape::Stagewise;
    else if (v1_narrow_regime(chains, ch, opt))
        P.shape = V1Shape::Tiny;
    else
        P.shape = opt.fold && !P.fast ? V1Shape::Latency : V1Shape::LatencyUnfolded;
    // the search progress word is (pass << 16) + rows: rows of a pass must stay below 2^16, else the stagewise search runs
    // (and, in the tiny regime, the four-lane converge launch behind it all the same)
    P.fusedSearch = P.fused() && frameSize / 8 < 65536u;
    const bool tiny = P.shape == V1Shape::Tiny;
    P.split = tiny && opt.splitCoder && (chains + 63) / 64 * 64 <= kSplitCoderMaxChains && v1_split_at(frameSize) >= 48;
    P.overlap = tiny && ch == 2 && !P.fast && opt.overlapPos && maxSegPackets > 1 && P.fusedSearch;
    return P;
}

const char *v1_regime_name(V1Shape shape)
{
    switch (shape) {
    case V1Shape::Lane: return "lane";
    case V1Shape::Tiny: return "tiny";
    case V1Shape::Latency:
    case V1Shape::LatencyUnfolded: return "latency";
    case V1Shape::Stagewise: return "stagewise";
    case V1Shape::Throughput: return "throughput";
    }
    return "";
}

hipError_t launch_encode_v1(uint32_t depth, uint32_t channels, const V1Args &A, const V1Plan &P, bool initState, const PackArgs &pa,
                            const V1Streams &vs, uint32_t numPackets, uint32_t maxSegPackets, hipStream_t st, hipEvent_t *ev)
{
    if (initState)
        ALAC_TRY(launch_kernel(k_init_state, dim3((A.S.numSegments * 64 + 255) / 256), dim3(256), st, A.state, A.S.numSegments));
#define V1_CASE(D)                                                                                   \
    case D:                                                                                          \
        return channels == 2 ? launch_v1_typed<D, 2>(A, P, numPackets, maxSegPackets, st, ev, pa, vs) \
                             : launch_v1_typed<D, 1>(A, P, numPackets, maxSegPackets, st, ev, pa, vs);
    switch (depth) {
        V1_CASE(16)
        V1_CASE(20)
        V1_CASE(24)
        V1_CASE(32)
    default: return hipErrorInvalidValue;
    }
#undef V1_CASE
}

}  // namespace alacdev
