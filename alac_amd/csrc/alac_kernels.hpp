// alac_kernels.hpp — argument blocks and launchers shared by the kernels and the C-ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

namespace alacdev {

// Every function that enqueues work returns hipError_t: the status of the FIRST runtime call or kernel launch in it that
// failed, behind which it enqueues nothing more.  ALAC_TRY passes such a status up; launch_kernel is the one
// place a kernel is launched from, and reads the launch's own status before any other call can overwrite it.
#define ALAC_TRY(call)                          \
    do {                                        \
        const hipError_t try_e_ = (call);       \
        if (try_e_ != hipSuccess) return try_e_; \
    } while (0)
// (k_lpc alone sizes its LDS at launch)
template <typename K, typename... Args>
inline hipError_t launch_kernel_lds(K kernel, dim3 grid, dim3 block, size_t ldsBytes, hipStream_t st, const Args &...args)
{
    hipLaunchKernelGGL(kernel, grid, block, ldsBytes, st, args...);
    return hipGetLastError();
}
template <typename K, typename... Args>
inline hipError_t launch_kernel(K kernel, dim3 grid, dim3 block, hipStream_t st, const Args &...args)
{
    return launch_kernel_lds(kernel, grid, block, 0, st, args...);
}

// per-channel part of a packet record
struct ChanRec {
    uint32_t bits;      // entropy-coded bits of this channel
    uint16_t num;       // numU / numV
    uint16_t pad;
    int16_t coefs[8];   // header coefficients (row state before the final pass)
};
// one per packet, written by the encode kernel, read by the packer
struct PacketRec {
    uint32_t numSamples;
    uint32_t escape;
    uint32_t mixRes;
    uint32_t totalBits;
    ChanRec c[2];
};
static_assert(sizeof(PacketRec) == 64, "PacketRec layout");
// LPC mode (option "lpc", alac_lpc.hip): the header of a channel whose coefficients were computed from the packet's PCM,
// [packet][2]; num == 0: the channel keeps Apple's header (PacketRec, denShift kDenShift)
constexpr int kLpcMaxOrder = 30;
struct LpcChan {
    uint16_t den;
    uint16_t num;
    int16_t coefs[kLpcMaxOrder];
};
static_assert(sizeof(LpcChan) == 64, "LpcChan layout");

struct EncodeArgs {
    const uint8_t *pcm;
    const uint32_t *numSamples;  // nullable
    const uint32_t *segFirst;    // nullable
    uint32_t numSegments;
    uint32_t frameSize;
    int16_t *state;              // nullable
    int32_t stateIn;
    int32_t *pred;               // [frameSize/8][predStride] search residual scratch
    uint64_t predStride;
    uint32_t *bitWords;          // [packet][2][wcap] per-channel bit strings
    uint32_t wcap;
    PacketRec *recs;
    uint32_t *packetBytes;
    // alac_hip_encode_segmented hands the segment table over UNVALIDATED (no host read-back): every kernel that forms a
    // packet index from it tests the entry against these two bounds (a segment that fails them has no packets), and
    // k_check_segments raises *segBad (device word) for k_finalize / k_scan_sizes / k_pack, which then produce nothing.
    uint32_t numPackets;
    uint32_t segMax;             // longest segment the caller promised (0xffffffff: table validated on the host)
    uint32_t *segBad;            // nullable
};

struct PackArgs {
    const uint8_t *pcm;
    const PacketRec *recs;
    const uint32_t *bitWords;
    uint32_t wcap;
    uint32_t frameSize;
    const uint64_t *offsets;
    uint8_t *out;
    const uint32_t *segBad;      // nullable; != 0: the segment table was refused on the device — pack nothing
    const LpcChan *lpc = nullptr; // nullable (LPC mode only): per packet and channel header overrides
};

// LPC mode, after the regular pipeline has encoded every packet as its own segment (alac_lpc.hip)
struct LpcArgs {
    const uint8_t *pcm;
    uint32_t frameSize;
    PacketRec *recs;
    uint32_t *packetBytes;
    uint32_t *bitWords;
    uint32_t wcap;
    LpcChan *lpc;  // [numPackets][2]
};
// one workgroup per packet; dynamic LDS channels * frameSize * 4 bytes (the caller keeps it <= 64 KB)
hipError_t launch_lpc(uint32_t depth, uint32_t channels, const LpcArgs &a, uint32_t numPackets, hipStream_t st);

// Stage timing: when `ev` is non-null, ev[i] is recorded BEFORE stage i and ev[kNumStages] after the
// last one (stages that do not run in a given configuration record back-to-back events).
enum EncodeStage {
    kStageLms1 = 0,   // LPC+mix, mixRes search passes
    kStageGol1,       // Golomb counts of those passes
    kStageLms2,       // LPC+mix, numUV converge passes
    kStageGol2,       // Golomb counts
    kStageLms3,       // LPC+mix, final pass
    kStageGol3,       // Golomb coder, final
    kStageScan,       // finalize + exclusive scan of packet sizes
    kStagePack,       // packer
    kNumStages
};

// lane-per-chain encoder (alac_encode.hip): everything fused in one kernel (recorded as kStageLms3)
hipError_t launch_encode(uint32_t depth, uint32_t channels, const EncodeArgs &ea, const PackArgs &pa,
                         uint32_t numPackets, hipStream_t st, hipEvent_t *ev);
// finalize is the caller's; this launches the size scan and the packer (records ev[kStageScan..])
hipError_t launch_scan_pack(uint32_t depth, uint32_t channels, uint32_t *packetBytes, const PackArgs &pa,
                            uint32_t numPackets, hipStream_t st, hipEvent_t *ev, bool recordScan = true);

// tap-parallel pipeline (alac_encode_v1.hip)
// In-launch producer -> consumer hand-offs (alac_encode_v1.hip RowWait, alac_decode_v1.hip k_dec_fused): a consumer
// whose bounded spin runs out has NOT seen its rows.  It raises *err (a host-mapped word the context checks at the next
// synchronize: the call then fails with kALAC_MemFullError instead of returning corrupt packets) and, in the decoder,
// marks its packets kALAC_ParamError.  `lose` is the test switch ALAC_HIP_DEBUG_LOSE_HANDOFF=1: producers never publish.
struct HandoffCtl {
    uint32_t *err = nullptr;
    uint32_t spinLimit = 1u << 22;
    uint32_t lose = 0;
};

// Per-context switches that select code paths (alac_hip_set_option; the ALAC_HIP_* environment variables of the same
// names are only the DEFAULTS a context starts from, read once in alac_hip_create).  -1 = automatic (chosen per call
// from the batch shape).
constexpr int32_t kPubEveryDefault = 1;
struct AlacOptions {
    int32_t thru = -1;         // "thru"         ALAC_HIP_THRU        encode: throughput (1) / latency (0) regime, -1 = by batch size
    int32_t narrow = -1;       // "narrow"       ALAC_HIP_NARROW      four lanes per chain, -1 = by batch size (v1_narrow_regime)
    int32_t splitCoder = 1;    // "split_coder"  ALAC_HIP_SPLIT_CODER tiny batches: final coder of a chain on two waves
    int32_t overlapPos = 1;    // "overlap_pos"  ALAC_HIP_OVERLAP_POS chained batches: position p + 1's search beside p's final pass
    int32_t fused = 1;         // "fused"        ALAC_HIP_FUSED       producer/consumer launches (latency regime); 0 = one kernel per stage
    int32_t pubEvery = kPubEveryDefault;  // "pub_every" ALAC_HIP_PUB_EVERY  fused launches: producers publish every 1 / 2 / 4 / 8 tiles (and every tile
                               // at the end of a pass)
    int32_t fold = 1;          // "fold"         ALAC_HIP_FOLD        latency regime: decision and packet sizes inside the final launch
    int32_t fastMode = 0;      // "fast_mode"    (no env)             ALACEncoder::SetFastMode: stereo elements without the search (EncodeStereoFast)
    int32_t laneEncoder = 0;   // "encoder_lane" ALAC_HIP_ENCODER=lane first-generation lane-per-chain encoder
    int32_t laneDecoder = 0;   // "decoder_lane" ALAC_HIP_DECODER=lane first-generation decoder
    int32_t decFused = -1;     // "dec_fused"    ALAC_HIP_DEC_FUSED   decode: entropy wave + its predictor waves in one launch, -1 = by batch size
    int32_t decPair = 1;       // "dec_pair"     ALAC_HIP_DEC_PAIR    decode, separate launches, 16-bit stereo: the predictor lanes of a packet un-mix and write the PCM
    int32_t decDirect = 1;     // "dec_direct"   ALAC_HIP_DEC_DIRECT  decode, separate launches: read the caller's stream directly (no staged
                               // copy): 0 never, 1 from kDecDirectPackets on, 2 whenever legal
    int32_t stageTaps = 1;     // "stage_taps"   ALAC_HIP_STAGE_TAPS  stage-level pc_block: tap-parallel kernel for 5..30 taps
    int32_t loseHandoff = 0;   // "debug_lose_handoff" ALAC_HIP_DEBUG_LOSE_HANDOFF  TEST switch: producers never publish (results invalid by design)
    int32_t lpc = 0;           // "lpc"          (no env)             independent packets with per-packet LPC coefficients (alac_lpc.hip)
    int32_t debugWaves = 0;    // "debug_waves"  wave placement / timing stamps of the fused final launch into the workspace (tools/wave_map.py)
};
AlacOptions alac_options_from_env();
struct AlacOptionKey {
    const char *name;
    const char *env;  // the ALAC_HIP_* variable that supplies the default (nullptr: none)
    int32_t AlacOptions::*slot;
    int32_t lo, hi;  // accepted values
    bool pow2 = false;  // ... of which only the powers of two
};
const AlacOptionKey *alac_option_keys(uint32_t *count);
const AlacOptionKey *alac_option_find(const char *key);  // nullptr for an unknown key
bool alac_option_accepts(const AlacOptionKey &k, long v);

// side stream and fork/join events (owned by the context): the second packet class of the throughput regime's final pass runs
// beside the first, and consecutive packet positions of a chained tiny batch alternate between the two streams
// (the launcher, launch_encode_v1, is declared with its argument block in alac_encode_v1_types.hpp)
constexpr uint32_t kSideEvents = 2;
struct V1Streams {
    hipStream_t side[1];
    hipEvent_t fork, stagger[kSideEvents], join[kSideEvents];
};
// stage events of one timed call: block 0 = predictor / Golomb stages, block 1 = finalize + scan + pack
constexpr uint32_t kEventBlocks = 2;
// *err = 1 (system scope) unless segFirst[0 .. numSegments] ascends inside [0, numPackets] with no step above maxSeg
hipError_t launch_check_segments(const uint32_t *segFirst, uint32_t numSegments, uint32_t numPackets, uint32_t maxSeg, uint32_t *err,
                                 uint32_t *segBad,
                                 hipStream_t st);
// What one mono / stereo encode call launches, decided once on the host (v1_plan, alac_encode_v1.hip):
//  Lane             the first-generation lane-per-chain encoder (option encoder_lane)
//  Tiny             four lanes per chain, producer/consumer launches, the final coder split over two waves where it fits
//  Latency          two lanes per chain, producer/consumer launches, the final launch decides and sizes the packets (fold)
//  LatencyUnfolded  the same without the fold (option fold = 0, or fast mode): k_decide2 and k_finalize stay
//  Stagewise        one kernel per stage (option fused = 0)
//  Throughput       one lane per chain, plain stores, the final pass per packet class
enum class V1Shape { Lane, Tiny, Latency, LatencyUnfolded, Stagewise, Throughput };
struct V1Plan {
    V1Shape shape;
    bool fast;         // stereo SetFastMode: k_decide_fast in place of every search pass
    bool fusedSearch;  // Tiny / Latency: the stereo mixRes search in one launch (its progress word counts rows below 2^16)
    bool split;        // Tiny: the final coder of a chain on two waves
    bool overlap;      // chained Tiny batch: the search of packet position p + 1 beside the final pass of p
    bool fused() const { return shape == V1Shape::Tiny || shape == V1Shape::Latency || shape == V1Shape::LatencyUnfolded; }
};
// channels: of the stream, > 2 counts as 2 (its elements are encoded as mono / stereo batches)
V1Plan v1_plan(uint32_t channels, uint32_t numSegments, uint32_t maxSegPackets, uint32_t frameSize, const AlacOptions &opt);
const char *v1_regime_name(V1Shape shape);  // what alac_hip_encode_regime reports
// the split coder's buffers exist in the workspace up to this many chains (rounded up to 64)
constexpr uint32_t kSplitCoderMaxChains = 4096;
// the second wave of the split coder starts coding at residual splitAt (whole 48-residual iterations, ~2/3 of the frame)
inline uint32_t v1_split_at(uint32_t frameSize) { return (frameSize * 2 / 3) / 48 * 48; }

// ---- decode ----
struct DecChan {
    uint16_t mode, denShift, pbFactor, num;
    int16_t coefs[32];
};
struct DecRec {
    uint32_t numSamples;
    uint32_t escape;
    int32_t mixBits, mixRes;
    uint32_t bytesShifted;
    uint32_t elementChannels;  // 1 (SCE/LFE) or 2 (CPE)
    uint64_t shiftPos;         // bit position of the shift-off section inside the packet
    int32_t status;            // of the whole packet in element record 0
    uint32_t pad;              // second-generation decoder: first payload bit of the element
    uint32_t chanIndex;        // first output channel of this element (lane decoder, element sequences)
    uint32_t pad2;
    DecChan c[2];
};

struct DecodeArgs {
    const uint8_t *stream;
    const uint64_t *offsets;
    uint32_t numPackets;
    uint32_t frameSize, bitDepth, numChannels;
    uint32_t mb, pb, kb;
    uint32_t maxElems;  // element records per packet (lane decoder): numChannels, a stream may be all SCE / LFE elements
    DecRec *recs;       // [maxElems][numPackets]
    const uint32_t *gate = nullptr;  // lane decoder as a fallback: its kernels do nothing unless *gate != 0
    HandoffCtl ho;
    int32_t optFused = -1, optPair = 1, optDirect = 1;  // AlacOptions::decFused / decPair / decDirect (host-side launch choices)
    int32_t *resid;  // [ch][frameSize][numPackets] residuals, then samples, in place
    uint8_t *pcmOut;  // verify mode: the caller's EXPECTED PCM, only ever read; float mode: the planar float32 output (alac_verify.hpp)
    uint32_t *numSamplesOut;
    int32_t *statusOut;
    // Each mode's own word shares one slot, and the mode sits in what was the struct's tail padding.  A mode with more words
    // than fit here (verify-float, int) carries them in a PcmModeArgs block beside this struct (below).
    union {
        // verify mode (alac_hip_verify): [numPackets] lowest sample-frame whose bytes differ, lowered with atomicMin by every
        // store site of the PCM (PCM_PUT, alac_verify.hpp), which loads and compares instead of storing
        uint32_t *firstMismatch = nullptr;
        uint64_t channelStride;  // float mode (alac_hip_decode_float): floats between two channels' rows of pcmOut
    };
    uint32_t frameBytes = 0;  // verify mode: bytes of one whole output frame (all channels)
    uint32_t pcmMode = 0;     // PcmMode (alac_verify.hpp): what the PCM store sites do
};
// by value in the kernel-argument segment (inside DecV1Args too): the compiled kernels read these offsets
static_assert(sizeof(DecodeArgs) == 144 && offsetof(DecodeArgs, pcmOut) == 104 && offsetof(DecodeArgs, firstMismatch) == 128 &&
                  offsetof(DecodeArgs, channelStride) == 128 && offsetof(DecodeArgs, frameBytes) == 136 &&
                  offsetof(DecodeArgs, pcmMode) == 140,
              "DecodeArgs layout");

struct PcmModeArgs;  // `pm` (below): the words of the call's PCM mode that do not fit in DecodeArgs
hipError_t launch_decode(const DecodeArgs &da, const PcmModeArgs &pm, hipStream_t st);
// verify mode (alac_verify.hip): firstMismatch[p] = ~0, *bad = 0 in front of the decode; after it, packets of non-zero status
// get 0, packets whose decoded frame count differs from the expected one min(decoded, expected), and *bad counts the packets
// left with a mismatch (numSamplesExpected null = every packet frameSize frames)
hipError_t launch_verify_init(uint32_t *firstMismatch, uint32_t numPackets, uint32_t *bad, hipStream_t st);
hipError_t launch_verify_finish(const int32_t *status, const uint32_t *numSamplesDecoded, const uint32_t *numSamplesExpected,
                                uint32_t frameSize, uint32_t numPackets, uint32_t *firstMismatch, uint32_t *bad, hipStream_t st);
// second generation (alac_decode_v1.hip): `words` = capWords uint32 of scratch for the re-staged stream, `plane` =
// numPackets * numChannels * frameSize int32, `prog` = 2 * numPackets + 2 uint32 (progress words of the fused launch;
// chain list and its two counters where the stages are separate launches)
// mismatch (nullable): device counter of the packets whose elements are not the expected sequence (status -4), cleared and
// counted by the pipeline itself
hipError_t launch_decode_v1(const DecodeArgs &da, const PcmModeArgs &pm, uint32_t *words, uint64_t capWords, int32_t *plane,
                            uint32_t *prog, hipStream_t st, uint32_t *mismatch);

// ---- > 2 channels (alac_multichannel.hip): a packet is a sequence of mono / stereo elements ----
struct McElement {
    uint32_t first;     // channel index of the element's first channel
    uint32_t channels;  // 1 (ID_SCE) or 2 (ID_CPE)
    uint32_t tag;       // element type (3 bits) << 4 | instance tag (4 bits)
};
constexpr uint32_t kMaxChannels = 8;
// the element sequence of a channel count (sChannelMaps, codec/ALACEncoder.cu:97-107); returns the count
uint32_t channel_elements(uint32_t numChannels, McElement *out);
struct McSpliceArgs {
    uint32_t numElements, numPackets;
    McElement el[kMaxChannels];
    const uint8_t *src[kMaxChannels];          // one-element packets of every element, back to back
    const uint64_t *srcOffsets[kMaxChannels];  // [numPackets + 1]
    uint32_t *elemBits;                        // [numElements][numPackets] scratch
    uint32_t *packetBytes;
    uint64_t *offsets;
    uint8_t *out;
};
// channels [first, first + channels) of an interleaved stream -> a compact mono / stereo stream (valid frames only)
hipError_t launch_mc_gather(const uint8_t *pcm, uint8_t *out, const uint32_t *numSamples, uint32_t numPackets,
                            uint32_t frameSize, uint32_t numChannels, uint32_t first, uint32_t channels, uint32_t bytesPerSample,
                            hipStream_t st);
// the per-packet sample counts and the segment table of `count` elements batched behind each other
// (sub-packet k * numPackets + p); either input may be null (then its output is not written)
hipError_t launch_mc_tables(const uint32_t *numSamples, uint32_t numPackets, const uint32_t *segFirst, uint32_t numSegments,
                            uint32_t count, uint32_t *numSamplesOut, uint32_t *segFirstOut, hipStream_t st);
// sizes + exclusive scan + bit-granular concatenation of the element packets
hipError_t launch_mc_splice(const McSpliceArgs &a, hipStream_t st);
hipError_t launch_scan_sizes(const uint32_t *sizes, uint64_t *offsets, uint32_t n, hipStream_t st, const uint32_t *segBad = nullptr);

// a stream of 3..8 channels on the second-generation decoder: one pass per element of the channel count's element
// sequence, element r of every packet decoded as the mono / stereo packet that starts where element r - 1 ended
// (elemBit: numPackets uint32 of scratch).  Packets whose elements are not that sequence end with status -4 and are
// counted in *mismatch (device): the caller then decodes the batch with launch_decode, which follows any sequence.
hipError_t launch_decode_v1_elements(const DecodeArgs &da, const PcmModeArgs &pm, const McElement *el, uint32_t numElements,
                                     uint32_t *words, uint64_t capWords, int32_t *plane, uint32_t *prog, uint32_t *elemBit,
                                     uint32_t *mismatch, hipStream_t st);

// ---- float32 input (alac_float_in.hip): alac_hip_encode_float's quantize pass in front of the encoder ----
// sample i of channel c of packet p is in[c * channelStride + (p * frameSize + i) * frameStride]; pcm gets the packed
// interleaved integer PCM of every packet at the full-packet stride (frames at or behind min(numSamples[p], frameSize) are
// not read and staged as zero); clipped (nullable) gets the count of clipped samples per packet (zeroed by the launcher)
struct FloatInArgs {
    const float *in;
    uint64_t channelStride, frameStride;
    const uint32_t *numSamples;  // null: every packet frameSize frames
    uint32_t numPackets, frameSize, channels;
    uint8_t *pcm;
    uint32_t *clipped;
};
// TPDF dither in front of the rounding (alac_hip_encode_float_dither; depth 16, 20 or 24): the sample at stream frame
// t = origin[p] + i (origin null: p * frameSize) of channel c gets the dither Philox4x32-10 gives for counter (t >> 1, c),
// half of its four words by t's parity.  roundKey: the ten round keys of the seed (philox_round_keys), the same for every
// sample, so the kernel reads them as scalars
struct FloatDitherArgs {
    const uint64_t *origin;  // [numPackets] or null
    uint32_t roundKey[10][2];
};
void philox_round_keys(uint64_t seed, uint32_t (&roundKey)[10][2]);
// how a float pass walks its input; a lane takes 4 consecutive frames that start at a multiple of 4
enum FloatLayout : int {
    kFloatPlanar = 0,       // frameStride 1: each channel's row contiguous (16-byte loads per channel)
    kFloatInterleaved = 1,  // channelStride 1, frameStride CH: frames contiguous (16-byte loads over the frame)
    kFloatGeneral = 2,      // any strides, any channel count: one load per sample
};
hipError_t launch_float_to_pcm(uint32_t depth, const FloatInArgs &a, hipStream_t st, const FloatDitherArgs *dither = nullptr);

// ---- integer input (alac_pcm_in.hip): alac_hip_pcm_requantize, the conversion pass of alac_hip_encode_int ----
// the container of sample i of channel c of packet p is at index c * channelStride + (p * frameSize + i) * frameStride of
// in (containers of containerBytes bytes: 2 int16, 3 packed little-endian, 4 int32); srcBits of it are significant, left-
// or right-justified (alac_hip_int_source).  pcm, numSamples and clipped as in FloatInArgs.
struct PcmInArgs {
    const void *in;
    uint64_t channelStride, frameStride;
    const uint32_t *numSamples;  // null: every packet frameSize frames
    uint32_t numPackets, frameSize, channels;
    uint32_t containerBytes, srcBits, leftJustified;
    uint8_t *pcm;
    uint32_t *clipped;
};
// the vector layouts of a pass over containers (1 or 2 channels): planar and interleaved int32 or float32 with 16-byte loads
// at every group of 4 frames, planar and interleaved int16 with 8-byte loads, interleaved packed 3-byte containers with dword
// loads
inline FloatLayout pcm_in_layout(const void *in, uint32_t containerBytes, uint32_t channels, uint64_t channelStride,
                                 uint64_t frameStride)
{
    const uintptr_t align = containerBytes == 4 ? 16 : containerBytes == 2 ? 8 : 4;
    if (channels > 2 || ((uintptr_t)in & (align - 1))) return kFloatGeneral;
    if (channels == 1) return frameStride == 1 ? kFloatPlanar : kFloatGeneral;
    if (channelStride == 1 && frameStride == 2) return kFloatInterleaved;
    if (containerBytes != 3 && frameStride == 1 && channelStride % 4 == 0) return kFloatPlanar;
    return kFloatGeneral;
}
// the one ladder from a layout and a channel count to the <CH, LAYOUT> pair of a pass's kernels: f(CH, LAYOUT), both
// std::integral_constant, CH 0 in the general layout
template <typename F>
inline hipError_t dispatch_layout(FloatLayout layout, uint32_t channels, F f)
{
    using std::integral_constant;
    if (layout == kFloatGeneral) return f(integral_constant<int, 0>(), integral_constant<int, kFloatGeneral>());
    if (channels == 1) return f(integral_constant<int, 1>(), integral_constant<int, kFloatPlanar>());
    if (layout == kFloatInterleaved) return f(integral_constant<int, 2>(), integral_constant<int, kFloatInterleaved>());
    return f(integral_constant<int, 2>(), integral_constant<int, kFloatPlanar>());
}
// depth: the target depth b.  dither (b < srcBits only): TPDF by the integer rule of include/alac_hip.h
hipError_t launch_pcm_requantize(uint32_t depth, const PcmInArgs &a, hipStream_t st, const FloatDitherArgs *dither = nullptr);

// ---- float32 probe (alac_float_probe.hip): alac_hip_float_probe's one pass over the floats ----
// the sample of channel c and frame t is in[c * channelStride + t * frameStride]; segment s = frames [segFirst[s],
// segFirst[s + 1]) adds to reports[s] (8 uint32 per segment: alac_hip_float_report).  segFirst: device table
// [numSegments + 1], ascending inside [lo, hi]; null: one segment [lo, hi).  Only frames in [lo, hi) are read.
struct FloatProbeArgs {
    const float *in;
    uint64_t channelStride, frameStride;
    uint64_t lo, hi;           // first frame of the first segment, end of the last one
    const uint64_t *segFirst;  // nullable
    uint32_t numSegments, channels;
    uint32_t *reports;
};
// zeroes the reports, then (hi > lo) the pass
hipError_t launch_float_probe(const FloatProbeArgs &a, hipStream_t st);

// ---- integer probe (alac_int_probe.hip): alac_hip_int_probe's one pass over the containers ----
// the container of channel c and frame t is at index c * channelStride + t * frameStride of in (containers as in PcmInArgs);
// segments, [lo, hi) and reports (8 uint32 per segment: alac_hip_int_report) as in FloatProbeArgs
struct IntProbeArgs {
    const void *in;
    uint64_t channelStride, frameStride;
    uint64_t lo, hi;
    const uint64_t *segFirst;  // nullable
    uint32_t numSegments, channels;
    uint32_t containerBytes, srcBits, leftJustified;
    uint32_t *reports;
};
// zeroes the reports, then (hi > lo) the pass
hipError_t launch_int_probe(const IntProbeArgs &a, hipStream_t st);

// ---- CRC-32 of PCM (alac_pcm_crc.hip): alac_hip_pcm_crc32's one pass over the bytes ----
// range s = bytes [ranges[2s], ranges[2s] + ranges[2s + 1]) of pcm adds to digests[4s ..] (alac_hip_pcm_digest).  ranges:
// device table, ascending and non-overlapping inside [lo, hi), lo = ranges[0], hi = the last range's end (the host checks);
// null: the one range [lo, hi).  Only bytes inside a range are read.
struct PcmCrcArgs {
    const uint8_t *pcm;
    uint64_t lo, hi;
    const uint64_t *ranges;  // nullable
    uint32_t numRanges;
    uint32_t *digests;
};
// what a lane, a wave and a block of k_pcm_crc take per iteration (alac_amd/capi.py mirrors them for the tests)
constexpr uint32_t kPcmCrcLaneShift = 6;
constexpr uint32_t kPcmCrcLaneBytes = 1u << kPcmCrcLaneShift;
constexpr uint32_t kPcmCrcWaveBytes = 64 * kPcmCrcLaneBytes;
constexpr uint32_t kPcmCrcBlockBytes = 4 * kPcmCrcWaveBytes;
// zeroes the digests, then (hi > lo) the pass, then the per-range finish
hipError_t launch_pcm_crc(const PcmCrcArgs &a, hipStream_t st);
// host: x^(8 * bytes) in GF(2)[x] / 0xEDB88320 (reflected), and the product of two such words
uint32_t crc_x8_pow(uint64_t bytes);
uint32_t crc_mul_host(uint32_t a, uint32_t b);

// ---- loudness (alac_loudness.hip): alac_hip_loudness_int / _float, BS.1770 energies per 100 ms and the sample peak ----
// The source as in IntProbeArgs (containerBytes 2, 3, 4) or FloatProbeArgs (containerBytes 0: float32).  Segment s = frames
// [segFirst[s], segFirst[s + 1]) is cut into chunks of L frames (the last one may be shorter) and its chunks into groups of
// kLoudGroup; rowBase / chunkBase / groupBase [numSegments + 1]: the first row, chunk and group of every segment in the
// call's arrays (device tables the host built; rows = floor(frames / hop), hop = L * chunksPerHop).
constexpr uint32_t kLoudGroup = 256;
struct LoudArgs {
    const void *in;
    uint64_t channelStride, frameStride;
    const uint64_t *segFirst, *rowBase, *chunkBase, *groupBase;
    uint32_t numSegments, channels;
    uint32_t containerBytes, srcBits, leftJustified;
    uint32_t L, chunksPerHop;
    uint32_t direct, pad;  // direct != 0: no pass stages its loads through LDS (ALAC_HIP_LOUDNESS_DIRECT=1, for measurements)
    uint64_t totalChunks, totalGroups, totalRows;
    double coef[10];  // {b0, b1, b2, a1, a2} of the shelf, then of the high-pass
    double M[16];     // the zero-input map of the filter's state over L frames, row-major
    double MG[16];    // ... over kLoudGroup * L frames
    double *state;    // [totalChunks][channels][4]: a chunk's end state from zero state, then its true start state
    double *gstate;   // [totalGroups][channels][4]: the same per group
    double *partial;  // [totalChunks][channels]: the chunk's sum of y^2
    double *energy;   // [totalRows][channels]
    uint32_t *reports;  // 8 words per segment: alac_hip_loudness_report
};
// the sample rates the loudness calls take: a multiple of 10 in [8 000, 384 000]
inline bool loud_rate_ok(uint32_t fs) { return fs >= 8000 && fs <= 384000 && fs % 10 == 0; }
// L of a sample rate: a divisor of hop = fs / 10 — the largest one <= 64, or where that is below 16 the smallest one >= 16
uint32_t loud_chunk_frames(uint32_t sampleRate);
// host: the two biquads of fs (fs checked by the caller), and M / MG of LoudArgs for chunks of L frames
void loud_filter_coefs(uint32_t sampleRate, double (&coef)[10]);
void loud_state_maps(const double (&coef)[10], uint32_t L, double (&M)[16], double (&MG)[16]);
// zeroes the reports, then the passes
hipError_t launch_loudness(const LoudArgs &a, hipStream_t st);

// ---- true peak (alac_true_peak.hip): alac_hip_true_peak_int / _float, BS.1770 annex 2 ----
// The source as in LoudArgs.  Segment s = frames [segFirst[s], segFirst[s + 1]) is cut into runs of `run` frames (the last one
// may be shorter), one lane each; chunkBase[numSegments + 1]: the first run of every segment among the call's runs.
constexpr uint32_t kTruePeakMaxTaps = 24, kTruePeakMaxCoefs = 36;
struct TruePeakArgs {
    const void *in;
    uint64_t channelStride, frameStride;
    const uint64_t *segFirst, *chunkBase;
    uint32_t numSegments, channels;
    uint32_t containerBytes, srcBits, leftJustified;
    uint32_t factor, run;  // F of the sample rate; true_peak_run(F)
    uint32_t direct;       // != 0: no staging through LDS (ALAC_HIP_TRUE_PEAK_DIRECT=1, for measurements)
    uint64_t totalChunks;
    double coef[kTruePeakMaxCoefs];  // phases 1 .. F-1, [F - 1][taps]
    uint64_t *channelPeak;           // [numSegments][channels]: the bits of the non-negative double
    uint32_t *reports;               // 8 words per segment: alac_hip_true_peak_report
};
// F of a sample rate the loudness calls take: 4 below 96 000, 2 below 192 000, 1 from there
inline uint32_t true_peak_factor(uint32_t fs) { return fs < 96000 ? 4u : fs < 192000 ? 2u : 1u; }
// taps per phase (K): 12, 24, and 0 where nothing is filtered
inline uint32_t true_peak_taps(uint32_t F) { return F == 4 ? 12u : F == 2 ? 24u : 0u; }
// the frames of a lane's run: with the K - 1 frames of history in front of them they fill whole slices of 16 frames
inline uint32_t true_peak_run(uint32_t F) { return F == 4 ? 53u : F == 2 ? 105u : 64u; }
// host: phases 1 .. F-1 of the 49-tap Hann-windowed sinc, [F - 1][taps]
void true_peak_coefs(uint32_t F, double (&coef)[kTruePeakMaxCoefs]);
// zeroes the reports and the channel peaks, then the pass and the finish
hipError_t launch_true_peak(const TruePeakArgs &a, hipStream_t st);

// ---- sample-rate conversion (alac_resample.hip): alac_hip_resample_int / _float ----
// The source as in LoudArgs.  Segment s = frames [segFirst[s], segFirst[s + 1]) gives the output frames [outFirst[s],
// outFirst[s + 1]) of every channel's row, cut into tiles of `tile` output frames (the last one may be shorter), one block
// each; tileBase[numSegments + 1]: the first tile of every segment among the call's tiles.
struct ResampleArgs {
    const void *in;
    uint64_t channelStride, frameStride;
    const uint64_t *segFirst, *outFirst, *tileBase;
    uint32_t numSegments, channels;
    uint32_t containerBytes, srcBits, leftJustified;
    uint32_t L, M, K;     // the plan of the rate pair (ResamplePlan)
    uint32_t tile, span;  // output frames of a tile; the input frames a tile needs at most (resample_span), what LDS holds
    uint64_t totalTiles;
    const double *coef;   // [K/2][L][2]: taps 2 kk and 2 kk + 1 of phase p at coef[(kk * L + p) * 2], 16-byte aligned
    float *out;           // channel c's output frame j at out[c * outChannelStride + j]
    uint64_t outChannelStride;
    uint32_t *reports;    // 8 words per segment: alac_hip_resample_report
};
// the plan of a rate pair by the rule of include/alac_hip.h; ok: the pair is one the calls take
struct ResamplePlan {
    uint32_t L, M, K;
    bool ok;
};
ResamplePlan resample_plan(uint32_t inRate, uint32_t outRate);
// output frames of a segment of n frames: ceil(n L / M)
inline uint64_t resample_out_frames(const ResamplePlan &p, uint64_t n) { return (n * p.L + p.M - 1) / p.M; }
// the input frames a tile of t output frames needs at most: its outputs' first and last centre frames and K - 1 around them
inline uint64_t resample_span(const ResamplePlan &p, uint64_t t) { return (t * p.M + p.L - 1) / p.L + p.K; }
// the output frames of a tile: 512, or as many as keep the tile's input span, as doubles of two channels (the most a block
// holds), inside kResampleLdsBytes of LDS (long filters: K grows with M / L, up to 3 840 at 48 : 1)
constexpr uint32_t kResampleTile = 512, kResampleLdsBytes = 64000;
inline uint32_t resample_tile(const ResamplePlan &p)
{
    uint32_t t = kResampleTile;
    while (t > 1 && resample_span(p, t) * 16 > kResampleLdsBytes) t /= 2;
    return t;
}
// host: the coefficients of a plan, computed once per pair and kept (the returned table lives as long as the process): [L][K],
// and behind it the same L * K doubles in the kernels' arrangement (ResampleArgs::coef)
const double *resample_coefs(const ResamplePlan &p);
// zeroes the reports, then the pass and the finish
hipError_t launch_resample(const ResampleArgs &a, hipStream_t st);

// ---- the words of the PCM modes that have more than fit in DecodeArgs (PcmMode, alac_verify.hpp) ----
// Sample i of channel c of packet p lives at index c * channelStride + (p * frameSize + i) * frameStride of DecodeArgs::pcmOut.
//  kPcmVerifyFloat (alac_hip_verify_float): pcmOut is the float32 source, only read, and only at frames
//      i < min(numSamplesExpected[p], frameSize); firstMismatch as DecodeArgs::firstMismatch in verify mode; dither != 0: the
//      source was quantized with TPDF dither by dz, as alac_hip_encode_float_dither
//  kPcmInt (alac_hip_decode_int): pcmOut is the destination, in containers of containerBytes bytes (2 int16, 3 packed
//      little-endian, 4 int32); the value is the decoded sample, sign-extended at the stream's depth, shifted left by `shift`
//      (left-justified: 8 * containerBytes - depth; right-justified at S bits: S - depth).  The other words are unused.
//  every other mode: never read (zero, but for the two tables the host files here for verify mode as well: verify_impl)
struct PcmModeArgs {
    uint32_t *firstMismatch;             // [numPackets]
    const uint32_t *numSamplesExpected;  // null: every packet frameSize frames
    uint64_t channelStride, frameStride;
    union {
        uint32_t dither;
        uint32_t containerBytes;
    };
    union {
        uint32_t pad;
        uint32_t shift;
    };
    FloatDitherArgs dz;
};
static_assert(sizeof(PcmModeArgs) == 128 && offsetof(PcmModeArgs, channelStride) == 16 && offsetof(PcmModeArgs, frameStride) == 24 &&
                  offsetof(PcmModeArgs, dither) == 32 && offsetof(PcmModeArgs, containerBytes) == 32 &&
                  offsetof(PcmModeArgs, pad) == 36 && offsetof(PcmModeArgs, shift) == 36 && offsetof(PcmModeArgs, dz) == 40,
              "PcmModeArgs layout");

// ---- stage-level ----
hipError_t launch_pc_block(const int32_t *in, int32_t *pc, uint32_t rows, uint32_t stride, int32_t num,
                           int16_t *coefs, int32_t numactive, uint32_t chanbits, uint32_t denshift,
                           bool decode, hipStream_t st, bool allowTaps = true);
// tap-parallel pc_block for any tap count (alac_stage_taps.hip); *_ok tells whether the shape is in its exact range
bool pc_block_taps_ok(int32_t num, int32_t na, uint32_t chanbits, uint32_t denshift);
hipError_t launch_pc_block_taps(const int32_t *in, int32_t *pc, uint32_t rows, uint32_t stride, int32_t num, int16_t *coefs,
                                int32_t na, uint32_t chanbits, uint32_t denshift, hipStream_t st);
hipError_t launch_dyn_comp(uint32_t mb0, uint32_t pb, uint32_t kb, const int32_t *pc, uint32_t rows,
                           uint32_t stride, int32_t numSamples, int32_t bitSize, uint8_t *bits,
                           uint32_t bytesStride, uint32_t *numBits, hipStream_t st);
hipError_t launch_dyn_decomp(uint32_t mb0, uint32_t pb, uint32_t kb, const uint8_t *bits,
                             uint32_t bytesStride, uint32_t rows, int32_t *pc, uint32_t stride,
                             int32_t numSamples, int32_t maxSize, uint32_t *numBits, int32_t *status,
                             hipStream_t st);

}  // namespace alacdev
