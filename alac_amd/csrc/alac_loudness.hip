// alac_loudness.hip — alac_hip_loudness_int / alac_hip_loudness_float: the K-weighted energy of every 100 ms of every channel
// (ITU-R BS.1770) and the sample peak of PCM where it lies, per segment of frames, and the host-only helpers that go with them
// (the filter's coefficients, the row count, the gated integrated loudness).  The rule is in include/alac_hip.h.
//
// The K-weighting filter is two biquads in series: an IIR, a serial chain along time.  It is linear, so the chain is cut:
// with s the four state words of a channel (two per biquad, transposed direct form II) at the start of a chunk of L frames,
//     s_end = M s + z        M: the zero-input map over L frames (4 x 4, the same for every chunk), z: the end state from s = 0
// Pass 1 filters every chunk from zero state (one lane per chunk) and keeps z; the scan carries the true states over the
// chunks of a segment (in groups of kLoudGroup chunks: per group from zero, over the groups with M^kLoudGroup, then per
// group again from its true state); pass 2 filters every chunk again from its true state and sums y^2; one lane per row and
// channel then adds the chunks of a hop in ascending order.  Nothing is summed with atomics, and every index a chunk, group
// or row is found by counts from its segment's first frame: the rows are the same bits whatever else the call holds.
// Reads through the loaders of alac_pcm_load.hpp in the layouts of pcm_in_layout, as the probes do; where a chunk's frames are
// contiguous bytes the loads go through LDS in coalesced 16-byte pieces (LoudStage).  The sources' rules and the staging are
// in alac_loud_source.hpp, shared with alac_true_peak.hip.
#include "alac_hip.h"
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_loud_source.hpp"
#include "alac_pcm_load.hpp"
#include "alac_probe_walk.hpp"

#include <cmath>
#include <cstdlib>
#include <vector>

namespace alacdev {

// one frame of one channel through both biquads; s: {shelf s1, s2, high-pass s1, s2}.  Every multiply-add is written as the
// fused operation it is: the order and the roundings are the same in every kernel and on the host, not the compiler's choice
__host__ __device__ __forceinline__ double kweight_step(const double (&c)[10], double x, double (&s)[4])
{
    const double y = fma(c[0], x, s[0]);
    s[0] = fma(c[1], x, fma(-c[3], y, s[1]));
    s[1] = fma(c[2], x, -(c[4] * y));
    const double w = fma(c[5], y, s[2]);
    s[2] = fma(c[6], y, fma(-c[8], w, s[3]));
    s[3] = fma(c[7], y, -(c[9] * w));
    return w;
}

// a state's four words, where the kernels keep them: two 16-byte halves (the workspace's arrays are 32-byte aligned)
struct LoudState {
    double2 lo, hi;
};
__device__ __forceinline__ LoudState loud_state(const double (&t)[4]) { return {{t[0], t[1]}, {t[2], t[3]}}; }

// t = M t + z, row by row, each row's products added left to right onto z
__device__ __forceinline__ void state_advance(const double (&M)[16], double (&t)[4], const LoudState z)
{
    const double t0 = t[0], t1 = t[1], t2 = t[2], t3 = t[3];
    t[0] = fma(M[3], t3, fma(M[2], t2, fma(M[1], t1, fma(M[0], t0, z.lo.x))));
    t[1] = fma(M[7], t3, fma(M[6], t2, fma(M[5], t1, fma(M[4], t0, z.lo.y))));
    t[2] = fma(M[11], t3, fma(M[10], t2, fma(M[9], t1, fma(M[8], t0, z.hi.x))));
    t[3] = fma(M[15], t3, fma(M[14], t2, fma(M[13], t1, fma(M[12], t0, z.hi.y))));
}

uint32_t loud_chunk_frames(uint32_t sampleRate)
{
    const uint32_t hop = sampleRate / 10;
    uint32_t L = 1;
    for (uint32_t d = 64; d >= 1; d--)
        if (hop % d == 0) {
            L = d;
            break;
        }
    if (L >= 16) return L;
    for (uint32_t d = 16; d < hop; d++)
        if (hop % d == 0) return d;
    return hop;
}

void loud_filter_coefs(uint32_t sampleRate, double (&c)[10])
{
    const double fs = (double)sampleRate, pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / fs);
        const double a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0, c[6] = -2.0, c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0;
        c[9] = (1.0 - K / Q + K * K) / a0;
    }
}

// column j of a map: the state the filter reaches from the unit state e_j over `frames` frames of zero input
static void zero_input_map(const double (&coef)[10], uint64_t frames, double (&M)[16])
{
    for (int j = 0; j < 4; j++) {
        double s[4] = {0, 0, 0, 0};
        s[j] = 1.0;
        for (uint64_t i = 0; i < frames; i++) (void)kweight_step(coef, 0.0, s);
        for (int i = 0; i < 4; i++) M[4 * i + j] = s[i];
    }
}

void loud_state_maps(const double (&coef)[10], uint32_t L, double (&M)[16], double (&MG)[16])
{
    zero_input_map(coef, L, M);
    zero_input_map(coef, (uint64_t)L * kLoudGroup, MG);
}

// the containers of frames [f0, f0 + 4), f0 a multiple of 4, of the CH channels of a vector layout
template <int CB, int CH, int LAYOUT>
__device__ __forceinline__ void loud_load_group(const LoudArgs &a, uint64_t f0, uint32_t (&v)[CH][4])
{
    if constexpr (LAYOUT == kFloatPlanar) {
#pragma unroll
        for (int c = 0; c < CH; c++) {
            int32_t e[4];
            load_run<CB, 4>((const uint8_t *)a.in + (c * a.channelStride + f0) * CB, e);
#pragma unroll
            for (int k = 0; k < 4; k++) v[c][k] = (uint32_t)e[k];
        }
    } else {
        int32_t e[4 * CH];
        load_run<CB, 4 * CH>((const uint8_t *)a.in + f0 * (CH * CB), e);
#pragma unroll
        for (int j = 0; j < 4 * CH; j++) v[j % CH][j / CH] = (uint32_t)e[j];
    }
}

// One lane: one chunk of L frames — all CH channels of it in a vector layout (CH 1 or 2: independent chains for the issue
// slots), one channel of it in the general layout (CH 0: a.channels lanes per chunk).
// Interleaved stereo and mono (the frames of a chunk are contiguous bytes): the loads are staged through LDS (LoudStage), one
// barrier in front of and one behind every slice's loads; every thread of the block runs every slice, with or without frames.
// Planar stereo and the general layout, and every layout under ALAC_HIP_LOUDNESS_DIRECT=1 (a.direct, the measurement switch):
// each lane loads its own frames — up to the first multiple of 4 and behind the last one by one, the groups of 4 between them
// with the vector loads of the layout.  Both ways a lane takes its frames in order: the same operations, the same bits.
// ENERGY false (pass 1): from zero state; the end state goes to a.state, and the chunk's peak word and non-finite count to
// its segment's report — one set of atomics per wave where the wave lies in one segment.  Every frame of a segment is in a
// chunk of this pass, the ones behind the last whole hop too.
// ENERGY true (pass 2): from the state the scan left in a.state; the sum of y^2 in frame order goes to a.partial.  Only the
// chunks of whole hops.
template <typename Src, int CH, int LAYOUT, bool ENERGY>
__global__ __launch_bounds__(256) void k_loud_pass(LoudArgs a)
{
    constexpr int NC = CH ? CH : 1;
    constexpr int CB = Src::kBytes;
    constexpr bool STAGED = LAYOUT == kFloatInterleaved || (LAYOUT == kFloatPlanar && CH == 1);
    constexpr int FB = NC * CB;
    const Src src(a);
    const uint32_t C = CH ? CH : a.channels;
    const uint32_t lanes = CH ? 1u : C;
    const uint64_t id = blockIdx.x * 256ull + threadIdx.x;
    const uint64_t g = id / lanes;
    const uint32_t c0 = (uint32_t)(id % lanes);
    const bool active = g < a.totalChunks;
    uint32_t peak = 0, nonfinite = 0, s = 0;
    uint64_t f0 = 0, f1 = 0, segFirst = 0, segEnd = 0;
    bool wanted = false;
    if (active) {
        s = probe_segment(a.chunkBase, a.numSegments, g);
        const uint64_t j = g - a.chunkBase[s];
        segFirst = a.segFirst[s], segEnd = a.segFirst[s + 1];
        f0 = segFirst + j * a.L;
        f1 = f0 + a.L < segEnd ? f0 + a.L : segEnd;
        wanted = !ENERGY || j < (a.rowBase[s + 1] - a.rowBase[s]) * a.chunksPerHop;
    }
    double st[NC][4], sum[NC];
    LoudState *slot = (LoudState *)a.state + (g * C + c0);
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const LoudState v = ENERGY && wanted ? slot[c] : LoudState{{0.0, 0.0}, {0.0, 0.0}};
        st[c][0] = v.lo.x, st[c][1] = v.lo.y, st[c][2] = v.hi.x, st[c][3] = v.hi.y;
        sum[c] = 0.0;
    }
    auto step = [&](const uint32_t(&raw)[NC]) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const double w = kweight_step(a.coef, src.value(raw[c], peak, nonfinite), st[c]);
            if (ENERGY) sum[c] = fma(w, w, sum[c]);
        }
    };
    bool direct = true;
    if constexpr (STAGED) {
        direct = a.direct != 0;  // (uniform)
        if (!direct) {
            __shared__ LoudStage<FB> S;
            const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
            const uint32_t frames = wanted ? (uint32_t)(f1 - f0) : 0u;
            const uint64_t before = (f0 - segFirst) * FB, behind = (segEnd - f1) * FB;
            const uint64_t first = (uint64_t)(uintptr_t)a.in + f0 * FB;
            S.first[w][lane] = first;
            S.total[w][lane] = frames * FB;
            S.slack[w][lane] = (uint32_t)(before < 15 ? before : 15) | (uint32_t)(behind < 15 ? behind : 15) << 8;
            const uint32_t slices = (a.L + LoudStage<FB>::kFrames - 1) / LoudStage<FB>::kFrames;
            for (uint32_t t = 0; t < slices; t++) {
                __syncthreads();  // the descriptors are written; the rows of the slice before are read
                loud_stage_slice(S, w, lane, t);
                __syncthreads();
                const uint32_t at = t * LoudStage<FB>::kFrames;
                const uint32_t n = frames > at ? (frames - at < LoudStage<FB>::kFrames ? frames - at : LoudStage<FB>::kFrames) : 0u;
                const uint8_t *row = S.rows[w] + lane * LoudStage<FB>::kRow + ((first + (uint64_t)at * FB) & 15);
#pragma unroll 4
                for (uint32_t i = 0; i < n; i++) {
                    uint32_t raw[NC];
#pragma unroll
                    for (int c = 0; c < NC; c++) raw[c] = (uint32_t)load_container<CB>(row, i * NC + c);
                    step(raw);
                }
            }
        }
    }
    if (direct && wanted) {
        auto one = [&](uint64_t f) {
            uint32_t raw[NC];
#pragma unroll
            for (int c = 0; c < NC; c++)
                raw[c] = (uint32_t)load_container<CB>(a.in, (c0 + c) * a.channelStride + f * a.frameStride);
            step(raw);
        };
        uint64_t f = f0;
        for (; f < f1 && (f & 3); f++) one(f);
        for (; f + 4 <= f1; f += 4) {
            uint32_t v[NC][4];
            if constexpr (LAYOUT != kFloatGeneral) {
                loud_load_group<CB, NC, LAYOUT>(a, f, v);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    v[0][k] = (uint32_t)load_container<CB>(a.in, c0 * a.channelStride + (f + k) * a.frameStride);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t raw[NC];
#pragma unroll
                for (int c = 0; c < NC; c++) raw[c] = v[c][k];
                step(raw);
            }
        }
        for (; f < f1; f++) one(f);
    }
    if (wanted) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            if (ENERGY) a.partial[g * C + c0 + c] = sum[c];
            else slot[c] = loud_state(st[c]);
        }
    }
    if constexpr (!ENERGY) {
        const uint32_t first = __shfl(s, 0);  // lane 0 is active wherever a lane of the wave is
        if (__ballot(active && s != first) == 0) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const uint32_t p2 = __shfl_xor(peak, m);
                peak = p2 > peak ? p2 : peak;
                nonfinite += __shfl_xor(nonfinite, m);
            }
            if ((threadIdx.x & 63) == 0 && active) loud_add(a.reports + 8ull * first, peak, nonfinite);
        } else if (active) {
            loud_add(a.reports + 8ull * s, peak, nonfinite);
        }
    }
}

// ---- the scan: s_{k+1} = M s_k + z_k over the chunks of a segment, per channel ----
// the chunks [k0, k1) of group q (of the call) of segment s, as indices into the call's chunks
__device__ __forceinline__ uint32_t loud_group_chunks(const LoudArgs &a, uint64_t q, uint64_t &k0, uint64_t &k1)
{
    const uint32_t s = probe_segment(a.groupBase, a.numSegments, q);
    const uint64_t base = a.chunkBase[s], end = a.chunkBase[s + 1];
    k0 = base + (q - a.groupBase[s]) * kLoudGroup;
    k1 = k0 + kLoudGroup < end ? k0 + kLoudGroup : end;
    return s;
}

// one lane per group and channel.  APPLY false: the group's end state from zero state, out of the chunks' z, into a.gstate.
// APPLY true: from the group's true start state in a.gstate, every chunk's z in a.state is replaced by its true start state.
template <bool APPLY>
__global__ __launch_bounds__(256) void k_loud_scan_group(LoudArgs a)
{
    const uint32_t C = a.channels;
    const uint64_t id = blockIdx.x * 256ull + threadIdx.x;
    const uint64_t q = id / C;
    const uint32_t c = (uint32_t)(id % C);
    if (q >= a.totalGroups) return;
    uint64_t k0, k1;
    (void)loud_group_chunks(a, q, k0, k1);
    LoudState *gs = (LoudState *)a.gstate + (q * C + c), *st = (LoudState *)a.state;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    if (APPLY) {
        const LoudState v = *gs;
        t[0] = v.lo.x, t[1] = v.lo.y, t[2] = v.hi.x, t[3] = v.hi.y;
    }
    for (uint64_t k = k0; k < k1; k++) {
        const LoudState z = st[k * C + c];
        if (APPLY) st[k * C + c] = loud_state(t);
        state_advance(a.M, t, z);
    }
    if (!APPLY) *gs = loud_state(t);
}

// one lane per segment and channel: the groups' end states from zero state are replaced by their true start states (MG
// moves a state over a whole group; only the last group of a segment may be shorter, and nothing follows it)
__global__ __launch_bounds__(256) void k_loud_scan_segment(LoudArgs a)
{
    const uint32_t C = a.channels;
    const uint64_t id = blockIdx.x * 256ull + threadIdx.x;
    const uint32_t c = (uint32_t)(id % C);
    if (id / C >= a.numSegments) return;
    const uint32_t s = (uint32_t)(id / C);
    LoudState *gs = (LoudState *)a.gstate;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (uint64_t q = a.groupBase[s]; q < a.groupBase[s + 1]; q++) {
        const LoudState z = gs[q * C + c];
        gs[q * C + c] = loud_state(t);
        state_advance(a.MG, t, z);
    }
}

// one lane per row and channel: the chunks of the hop, added in ascending order
__global__ __launch_bounds__(256) void k_loud_rows(LoudArgs a)
{
    const uint32_t C = a.channels;
    const uint64_t id = blockIdx.x * 256ull + threadIdx.x;
    const uint64_t r = id / C;
    const uint32_t c = (uint32_t)(id % C);
    if (r >= a.totalRows) return;
    const uint32_t s = probe_segment(a.rowBase, a.numSegments, r);
    const uint64_t k0 = a.chunkBase[s] + (r - a.rowBase[s]) * a.chunksPerHop;
    double e = 0.0;
    for (uint32_t i = 0; i < a.chunksPerHop; i++) e += a.partial[(k0 + i) * C + c];
    a.energy[r * C + c] = e;
}

// per segment: the fields of the report that are not collected, and the peak's word as a double
template <typename Src>
__global__ __launch_bounds__(256) void k_loud_finish(LoudArgs a)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.numSegments) return;
    const Src src(a);
    uint32_t *d = a.reports + 8ull * s;
    const double peak = src.peak_value(d[2]);
    d[0] = (uint32_t)a.rowBase[s];
    d[1] = (uint32_t)(a.rowBase[s + 1] - a.rowBase[s]);
    *(double *)(d + 2) = peak;
    d[6] = 0, d[7] = 0;
}

static bool loud_grid(uint64_t lanes, dim3 &grid)
{
    const uint64_t blocks = (lanes + 255) / 256;
    grid = dim3((uint32_t)blocks);
    return blocks >= 1 && blocks <= 0x7fffffffull;
}

template <typename Src>
static hipError_t launch_source(const LoudArgs &a, hipStream_t st)
{
    constexpr int CB = Src::kBytes;
    const uint32_t C = a.channels;
    dim3 grid;
    ALAC_TRY(hipMemsetAsync(a.reports, 0, (uint64_t)a.numSegments * 32, st));
    if (a.totalChunks) {
        const FloatLayout layout = pcm_in_layout(a.in, CB, C, a.channelStride, a.frameStride);
        auto pass = [&](auto energy) {
            return dispatch_layout(layout, C, [&](auto ch, auto lay) {
                constexpr int CH = decltype(ch)::value, LAYOUT = decltype(lay)::value;
                constexpr bool ENERGY = decltype(energy)::value;
                // pcm_in_layout names no planar layout of two rows of packed 3-byte containers
                if constexpr (CB == 3 && CH == 2 && LAYOUT == kFloatPlanar) return hipErrorInvalidValue;
                else {
                    if (!loud_grid(a.totalChunks * (CH ? 1u : C), grid)) return hipErrorInvalidValue;
                    return launch_kernel(k_loud_pass<Src, CH, LAYOUT, ENERGY>, grid, dim3(256), st, a);
                }
            });
        };
        ALAC_TRY(pass(std::false_type()));
        if (a.totalRows) {
            if (!loud_grid(a.totalGroups * C, grid)) return hipErrorInvalidValue;
            ALAC_TRY(launch_kernel(k_loud_scan_group<false>, grid, dim3(256), st, a));
            (void)loud_grid((uint64_t)a.numSegments * C, grid);
            ALAC_TRY(launch_kernel(k_loud_scan_segment, grid, dim3(256), st, a));
            (void)loud_grid(a.totalGroups * C, grid);
            ALAC_TRY(launch_kernel(k_loud_scan_group<true>, grid, dim3(256), st, a));
            ALAC_TRY(pass(std::true_type()));
            if (!loud_grid(a.totalRows * C, grid)) return hipErrorInvalidValue;
            ALAC_TRY(launch_kernel(k_loud_rows, grid, dim3(256), st, a));
        }
    }
    return launch_kernel(k_loud_finish<Src>, dim3((a.numSegments + 255) / 256), dim3(256), st, a);
}

hipError_t launch_loudness(const LoudArgs &args, hipStream_t st)
{
    LoudArgs a = args;
    const char *direct = getenv("ALAC_HIP_LOUDNESS_DIRECT");  // the measurement switch: no staging through LDS
    a.direct = direct && direct[0] == '1';
    const uint32_t S = a.srcBits, CB = a.containerBytes;
    if (a.numSegments == 0 || a.channels < 1 || a.channels > kMaxChannels || a.L == 0 || a.chunksPerHop == 0)
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

int32_t alac_hip_loudness_filter(uint32_t sample_rate, double *out)
{
    if (!out || !loud_rate_ok(sample_rate)) return ALAC_HIP_ParamError;
    double c[10];
    loud_filter_coefs(sample_rate, c);
    for (int i = 0; i < 10; i++) out[i] = c[i];
    return ALAC_HIP_noErr;
}

uint64_t alac_hip_loudness_rows(uint32_t sample_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                uint32_t num_segments)
{
    if (!loud_rate_ok(sample_rate) || num_segments == 0) return 0;
    const uint64_t hop = sample_rate / 10;
    if (!h_seg_first_frame) return num_segments == 1 ? total_frames / hop : 0;
    uint64_t rows = 0;
    for (uint32_t s = 0; s < num_segments; s++) {
        if (h_seg_first_frame[s] > h_seg_first_frame[s + 1]) return 0;
        rows += (h_seg_first_frame[s + 1] - h_seg_first_frame[s]) / hop;
    }
    return h_seg_first_frame[num_segments] > total_frames ? 0 : rows;
}

// BS.1770's channel weights in the channel order of the ALAC layout tag of a channel count
static const double *loud_default_weights(uint32_t channels)
{
    static const double w[8][8] = {{1}, {1, 1}, {1, 1, 1}, {1, 1, 1, 1}, {1, 1, 1, 1.41, 1.41}, {1, 1, 1, 1.41, 1.41, 0},
                                   {1, 1, 1, 1.41, 1.41, 1, 0}, {1, 1, 1, 1, 1, 1.41, 1.41, 0}};
    return w[channels - 1];
}

int32_t alac_hip_loudness_integrated(const double *h_energy, uint64_t num_blocks, uint32_t num_channels, uint32_t hop,
                                     const double *weights, double *out_lufs)
{
    if (!out_lufs || (!h_energy && num_blocks) || num_channels < 1 || num_channels > kMaxChannels || hop == 0)
        return ALAC_HIP_ParamError;
    *out_lufs = -HUGE_VAL;
    if (num_blocks < 4) return ALAC_HIP_noErr;
    const double *G = weights ? weights : loud_default_weights(num_channels);
    const uint64_t n = num_blocks - 3, C = num_channels;
    const double norm = 4.0 * (double)hop;
    std::vector<double> power(n);
    for (uint64_t j = 0; j < n; j++) {
        double p = 0.0;
        for (uint32_t c = 0; c < C; c++) {
            const double *e = h_energy + j * C + c;
            p += G[c] * ((e[0] + e[C] + e[2 * C] + e[3 * C]) / norm);
        }
        power[j] = p;
    }
    auto loudness = [](double p) { return -0.691 + 10.0 * std::log10(p); };  // p == 0: -inf
    auto gated_mean = [&](double gate, double &mean) {
        double sum = 0.0;
        uint64_t count = 0;
        for (uint64_t j = 0; j < n; j++) {
            const double l = loudness(power[j]);
            if (l > -70.0 && l > gate) sum += power[j], count++;
        }
        mean = count ? sum / (double)count : 0.0;
        return count != 0;
    };
    double mean;
    if (!gated_mean(-HUGE_VAL, mean)) return ALAC_HIP_noErr;
    if (!gated_mean(loudness(mean) - 10.0, mean)) return ALAC_HIP_noErr;
    *out_lufs = loudness(mean);
    return ALAC_HIP_noErr;
}
