// alac_capi.hip — the extern "C" boundary of libalac_hip.so (declared in include/alac_hip.h).
// Host-side only: argument checks, workspace carving, kernel launches.  No exceptions cross the
// boundary; every HIP failure becomes one of the reference's int32 status codes.
#include "alac_hip.h"
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_verify.hpp"
#include "alac_encode_v1_types.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace alacdev;

struct alac_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    std::string err;
    // optional per-stage timing: kEventBlocks blocks of kNumStages + 1 events per encode call, recorded on `stream`
    bool profile = false;
    std::vector<hipEvent_t> events;
    uint32_t profCalls = 0;
    std::vector<bool> profLane;  // per timed call: lane encoder, no predictor-stage events (block 0 unused)
    // side stream / events of the tap-parallel pipeline (V1Streams, created on first use)
    V1Streams vs{};
    bool vsReady = false;
    // second stream of the > 2-channel encoder (mono elements beside the stereo ones)
    hipStream_t mcStream = nullptr;
    hipEvent_t mcFork = nullptr, mcJoin = nullptr;
    bool mcReady = false;
    // error word of the in-launch hand-offs (HandoffCtl): pinned host memory the kernels write with a system-scope
    // store when a consumer's bounded wait runs out; read without a copy after a synchronize
    uint32_t *errHost = nullptr;
    uint32_t *errDev = nullptr;
    // code-path switches of this context (alac_hip_set_option); defaults from the ALAC_HIP_* environment at creation
    AlacOptions opt;
};

namespace alacdev {

static int env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

AlacOptions alac_options_from_env()
{
    AlacOptions o;
    o.thru = env_int("ALAC_HIP_THRU", o.thru);
    o.narrow = env_int("ALAC_HIP_NARROW", o.narrow);
    o.splitCoder = env_int("ALAC_HIP_SPLIT_CODER", o.splitCoder) != 0;
    o.overlapPos = env_int("ALAC_HIP_OVERLAP_POS", o.overlapPos) != 0;
    o.fused = env_int("ALAC_HIP_FUSED", o.fused) != 0;
    o.fold = env_int("ALAC_HIP_FOLD", o.fold) != 0;
    if (const char *e = getenv("ALAC_HIP_ENCODER")) o.laneEncoder = strcmp(e, "lane") == 0;
    if (const char *e = getenv("ALAC_HIP_DECODER")) o.laneDecoder = strcmp(e, "lane") == 0;
    if (const char *e = getenv("ALAC_HIP_DEC_FUSED")) o.decFused = *e ? (e[0] == '0' ? 0 : 1) : -1;
    o.decPair = env_int("ALAC_HIP_DEC_PAIR", o.decPair) != 0;
    o.decDirect = env_int("ALAC_HIP_DEC_DIRECT", o.decDirect) != 0;
    o.stageTaps = env_int("ALAC_HIP_STAGE_TAPS", o.stageTaps) != 0;
    o.loseHandoff = env_int("ALAC_HIP_DEBUG_LOSE_HANDOFF", o.loseHandoff) == 1;
    return o;
}

// key -> slot and the range alac_hip_set_option accepts (include/alac_hip.h documents exactly these)
const AlacOptionKey *alac_option_keys(uint32_t *count)
{
    static const AlacOptionKey table[] = {
        {"thru", &AlacOptions::thru, -1, 1},           {"narrow", &AlacOptions::narrow, -1, 1},
        {"split_coder", &AlacOptions::splitCoder, 0, 1}, {"overlap_pos", &AlacOptions::overlapPos, 0, 1},
        {"fused", &AlacOptions::fused, 0, 1},          {"fold", &AlacOptions::fold, 0, 1},
        {"fast_mode", &AlacOptions::fastMode, 0, 1},   {"encoder_lane", &AlacOptions::laneEncoder, 0, 1},
        {"decoder_lane", &AlacOptions::laneDecoder, 0, 1}, {"dec_fused", &AlacOptions::decFused, -1, 1},
        {"dec_pair", &AlacOptions::decPair, 0, 1},     {"dec_direct", &AlacOptions::decDirect, 0, 2},
        {"stage_taps", &AlacOptions::stageTaps, 0, 1},  {"lpc", &AlacOptions::lpc, 0, 1},
        {"debug_lose_handoff", &AlacOptions::loseHandoff, 0, 1}, {"debug_waves", &AlacOptions::debugWaves, 0, 1},
    };
    if (count) *count = (uint32_t)(sizeof(table) / sizeof(table[0]));
    return table;
}

const AlacOptionKey *alac_option_find(const char *key)
{
    if (!key) return nullptr;
    uint32_t n = 0;
    const AlacOptionKey *t = alac_option_keys(&n);
    for (uint32_t i = 0; i < n; i++)
        if (strcmp(t[i].name, key) == 0) return t + i;
    return nullptr;
}

}  // namespace alacdev

namespace {

int32_t fail(alac_hip_ctx *ctx, int32_t code, const char *what, hipError_t e = hipSuccess)
{
    if (ctx) {
        ctx->err = what;
        if (e != hipSuccess) {
            ctx->err += ": ";
            ctx->err += hipGetErrorString(e);
        }
    }
    return code;
}

bool format_ok(const alac_hip_format *f)
{
    if (!f) return false;
    if (!(f->bit_depth == 16 || f->bit_depth == 20 || f->bit_depth == 24 || f->bit_depth == 32)) return false;
    if (f->num_channels < 1 || f->num_channels > kMaxChannels) return false;
    if (f->frame_size == 0 || f->frame_size > (1u << 20)) return false;
    return true;
}

inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// the ALACSpecificConfig inside a cookie: ALACDecoder::Init skips legacy 'frma' and 'alac' atoms (codec/ALACDecoder.cu:123-134)
const uint8_t *cookie_config(const uint8_t *ck, uint32_t &size)
{
    for (const char *atom : {"frma", "alac"})
        if (size >= 12 && memcmp(ck + 4, atom, 4) == 0) {
            ck += 12;
            size -= 12;
        }
    return ck;
}

HandoffCtl handoff_ctl(const alac_hip_ctx *ctx)
{
    HandoffCtl h;
    h.err = ctx->errDev;
    h.lose = ctx->opt.loseHandoff ? 1u : 0u;  // test switch ("debug_lose_handoff"): producers never publish, consumers give up fast
    h.spinLimit = h.lose ? (1u << 8) : (1u << 22);
    return h;
}

// the context's second stream + fork / join events (mono elements beside stereo ones in the > 2-channel encoder), created on
// first use
bool ensure_second_stream(alac_hip_ctx *ctx)
{
    if (ctx->mcReady) return true;
    if (hipStreamCreateWithFlags(&ctx->mcStream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->mcFork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->mcJoin, hipEventDisableTiming) != hipSuccess)
        return false;
    ctx->mcReady = true;
    return true;
}

// after the stream has been synchronised: did a consumer of an in-launch hand-off give up?
int32_t check_handoff(alac_hip_ctx *ctx)
{
    if (!ctx->errHost) return ALAC_HIP_noErr;
    volatile uint32_t *w = (volatile uint32_t *)ctx->errHost;
    if (w[1] != 0) {  // k_check_segments: the caller's segment table contradicts the bound it gave
        w[1] = 0;
        w[0] = 0;
        return fail(ctx, ALAC_HIP_ParamError,
                    "d_seg_first is not ascending inside [0, num_packets] or a segment is longer than max_segment_packets: the "
                    "results of the calls since the last synchronize are invalid");
    }
    if (w[0] == 0) return ALAC_HIP_noErr;
    w[0] = 0;
    return fail(ctx, ALAC_HIP_MemFullError,
                "an in-launch producer/consumer hand-off timed out: the results of the calls since the last synchronize are invalid");
}

struct EncLayout {
    uint64_t recs, bitWords, pred, total;
    uint32_t wcap;
    uint64_t predStride;
    // tap-parallel pipeline: residual planes [sample][stream], decision scratch, working state
    uint64_t resA, resB, resC, bits1, cost2, state, flags, rowReady, cls, colChain;
    uint64_t bitWordsB, bitsB;  // tiny batches only (0: absent): second coder wave of the split final coder
    uint64_t segBad;            // one word: k_check_segments refused the caller's segment table (EncodeArgs::segBad)
    uint32_t chainsPad, colsPad;
};

EncLayout enc_layout(const alac_hip_format *f, uint32_t numPackets, uint32_t numSegments)
{
    EncLayout L;
    // escape size bounds what a compressed element may use (codec/ALACEncoder.cu:459,:538)
    const uint64_t escapeBits = (uint64_t)f->frame_size * f->bit_depth * f->num_channels + 32 + 16;
    // + 44 words: the written coder guards its slot 34 words before the end (alac_golomb.hpp, golf_open), and a channel that
    // gets there must by itself be longer than the escape size; a multiple of 4 words: 16-byte aligned channel slots.
    // The slot stride also decides how the coder's scattered stores (one word per lane and symbol in the latency regime,
    // ~10^11 L2 write requests per second) fall onto the L2 channels: measured at 10 000 packets, the final launch takes
    // 0.746 ms with 16 576-byte slots (16-bit stereo, this formula), 0.78-0.80 ms 32 or 256 bytes further, and 0.96 ms with
    // the 24 768 bytes the formula gives 24-bit stereo against 0.76 ms 16 bytes further — hence the extra group there.
    // ALAC_HIP_WCAP_PAD (words) adds to it for experiments.
    L.wcap = (uint32_t)(((escapeBits + 31) / 32 + 44 + 3) & ~3ull);
    if (f->bit_depth == 24) L.wcap += 4;
    if (const char *e = getenv("ALAC_HIP_WCAP_PAD")) L.wcap += (uint32_t)atoi(e) & ~3u;
    const uint64_t lanes = align_up((uint64_t)numSegments * f->num_channels, 64);
    L.predStride = lanes;
    uint64_t off = 0;
    L.recs = off;
    off = align_up(off + (uint64_t)numPackets * sizeof(PacketRec), 256);
    L.bitWords = off;
    // + one spare packet slot: lanes that own no packet write their (ignored) bit words there
    off = align_up(off + ((uint64_t)numPackets + 1) * 2 * L.wcap * 4, 256);
    L.pred = off;
    off = align_up(off + (uint64_t)(f->frame_size / 8 + 1) * lanes * 4, 256);
    L.chainsPad = (uint32_t)lanes;
    // +16 rows: the coder waves read whole 16-row blocks up to the wave's longest chain
    const uint64_t n8 = f->frame_size / 8 + 1 + 16;
    L.resA = off;
    off = align_up(off + (f->num_channels == 2 ? n8 * 5 * lanes * 4 : 0), 256);
    L.resB = off;
    off = align_up(off + n8 * 2 * lanes * 4, 256);
    // final residuals: columns handed out per packet class (k_class_assign), two regions padded to 64 -> up to 128 spare
    L.colsPad = (uint32_t)lanes + 256;  // the two class regions of the final pass are padded to whole waves
    L.resC = off;
    off = align_up(off + ((uint64_t)f->frame_size + 16) * L.colsPad * 4, 256);
    L.bits1 = off;
    off = align_up(off + 5 * lanes * 4, 256);
    L.cost2 = off;
    off = align_up(off + 2 * lanes * 4, 256);
    L.state = off;
    off = align_up(off + (uint64_t)numSegments * 128, 256);
    L.flags = off;  // one progress word per predictor wave (up to lanes / 16), twice: search and final launch of
                    // consecutive packet positions of a chained batch run side by side
    off = align_up(off + 2 * (lanes / 8 + 16) * 4, 256);
    L.rowReady = off;
    off = align_up(off + lanes * 4, 256);
    L.cls = off;  // ClassInfo + per-1024-packet class counts of the compaction
    off = align_up(off + 256 + ((uint64_t)numSegments / 1024 + 2) * 8, 256);
    L.colChain = off;
    off = align_up(off + (uint64_t)L.colsPad * 4, 256);
    // The smallest batches (<= kSplitCoderMaxChains: a chained file, a few hundred files side by side — the low end of the
    // four-lanes-per-chain regime, v1_narrow_regime): the final coder of a chain is split over two waves, the second one
    // writes here
    L.bitWordsB = L.bitsB = 0;
    if (lanes <= kSplitCoderMaxChains) {
        L.bitWordsB = off;
        off = align_up(off + ((uint64_t)numPackets + 1) * 2 * L.wcap * 4, 256);
        L.bitsB = off;
        off = align_up(off + ((uint64_t)numPackets + 1) * 2 * 4, 256);
    }
    L.segBad = off;
    off += 256;
    L.total = off;
    return L;
}

// option "encoder_lane" selects the fused lane-per-chain kernel (alac_encode.hip); default is the
// tap-parallel pipeline (alac_encode_v1.hip).  Both are HIP paths; there is no CPU path.
bool use_lane_encoder(const alac_hip_ctx *ctx) { return ctx->opt.laneEncoder != 0; }

// > 2 channels: the mono / stereo pipeline once per element over a gathered copy of its channels, then the splice
// (alac_multichannel.hip)
alac_hip_format element_format(const alac_hip_format *f, uint32_t channels)
{
    alac_hip_format e = *f;
    e.num_channels = channels;
    return e;
}

uint64_t max_output_bytes(const alac_hip_format *fmt, uint32_t num_packets)
{
    // escape elements: 7 + 16 + 32 + N*ch*depth bits each, + ID_END, rounded up; +8 so word stores may overhang
    const uint64_t elems = fmt->num_channels > 2 ? fmt->num_channels : 1;
    const uint64_t per = ((uint64_t)fmt->frame_size * fmt->num_channels * fmt->bit_depth + 55 * elems + 3 + 7) / 8;
    return align_up(per * num_packets + 8, 16);
}

// the elements of one type form one batch of count * numPackets one-element packets (sub-packet k * P + p)
struct McGroup {
    uint32_t channels, count, elem[kMaxChannels];
    uint64_t gather, sub, subBytes, out, outCap, sizes, offs, ns, seg, state;
};

struct McLayout {
    uint32_t numElements;
    McElement el[kMaxChannels];
    uint32_t groupOf[kMaxChannels], indexInGroup[kMaxChannels];
    McGroup g[2];  // [0] stereo elements, [1] mono elements
    uint64_t elemBits, total;
};

McLayout mc_layout(const alac_hip_format *f, uint32_t numPackets, uint32_t numSegments)
{
    McLayout M;
    M.numElements = channel_elements(f->num_channels, M.el);
    M.g[0].channels = 2;
    M.g[1].channels = 1;
    M.g[0].count = M.g[1].count = 0;
    for (uint32_t e = 0; e < M.numElements; e++) {
        McGroup &G = M.g[M.el[e].channels == 2 ? 0 : 1];
        M.groupOf[e] = M.el[e].channels == 2 ? 0 : 1;
        M.indexInGroup[e] = G.count;
        G.elem[G.count++] = e;
    }
    uint64_t off = 0;
    for (int gi = 0; gi < 2; gi++) {
        McGroup &G = M.g[gi];
        const alac_hip_format gf = element_format(f, G.channels);
        const uint64_t subPackets = (uint64_t)G.count * numPackets, subSegments = (uint64_t)G.count * numSegments;
        G.gather = off;
        off = align_up(off + subPackets * f->frame_size * G.channels * bytes_per_sample(f->bit_depth) + 64, 256);
        G.sub = off;
        G.subBytes = G.count ? enc_layout(&gf, (uint32_t)subPackets, (uint32_t)subSegments).total : 0;
        off = align_up(off + G.subBytes, 256);
        G.outCap = max_output_bytes(&gf, (uint32_t)subPackets);
        G.out = off;
        off = align_up(off + G.outCap + 16, 256);
        G.sizes = off;
        off = align_up(off + subPackets * 4, 256);
        G.offs = off;
        off = align_up(off + (subPackets + 1) * 8, 256);
        G.ns = off;
        off = align_up(off + subPackets * 4, 256);
        G.seg = off;
        off = align_up(off + (subSegments + 1) * 4, 256);
        G.state = off;
        off = align_up(off + subSegments * ALAC_HIP_STATE_INT16 * 2, 256);
    }
    M.elemBits = off;
    off = align_up(off + (uint64_t)M.numElements * numPackets * 4, 256);
    M.total = off;
    return M;
}

struct DecLayout {
    uint64_t recs, resid, words, capWords, prog, elemBit, mismatch, total;
    uint32_t maxElems;
};

// streamBytes = 0: every packet at its largest regular size (what an encoder of this library or Apple's can emit);
// a stream padded with ID_FIL / ID_DSE elements may be longer, and a caller who knows its length passes it
DecLayout dec_layout(const alac_hip_format *f, uint32_t numPackets, uint64_t streamBytes = 0)
{
    DecLayout L;
    uint64_t off = 0;
    L.recs = off;
    // a mono / stereo stream may still be a sequence of SCE / LFE elements (codec/ALACDecoder.cu:622-756): the lane
    // decoder keeps one record per channel
    L.maxElems = f->num_channels;
    off = align_up(off + (uint64_t)numPackets * L.maxElems * sizeof(DecRec), 256);
    L.resid = off;
    off = align_up(off + (uint64_t)f->num_channels * f->frame_size * numPackets * 4 + 256, 256);  // + block over-read
    L.prog = off;  // progress words of the fused launch / chain list, counters and pair list of the separate launches
    off = align_up(off + (uint64_t)numPackets * 28 + 64, 256);  // dec_lists (alac_decode_v1.hip): 7 n words + 16 counters
    L.elemBit = off;
    off = align_up(off + (uint64_t)numPackets * 4, 256);
    L.mismatch = off;
    off = align_up(off + 4, 256);
    // LAST: the stream re-staged as MSB-first words + 64 zero words (alac_decode_v1.hip).  Whatever the caller's
    // workspace holds beyond this offset is used, so a longer stream only needs a larger workspace.
    L.words = off;
    const uint64_t regular = (uint64_t)numPackets * max_output_bytes(f, 1);
    L.capWords = ((streamBytes > regular ? streamBytes : regular) + 3) / 4 + 64;
    off = align_up(off + L.capWords * 4, 256);
    L.total = off;
    return L;
}

// LPC mode: the header overrides of every packet and channel, behind the regular layout
uint64_t lpc_table_bytes(uint32_t numPackets) { return align_up((uint64_t)numPackets * 2 * sizeof(LpcChan), 256); }

bool use_lane_decoder(const alac_hip_ctx *ctx) { return ctx->opt.laneDecoder != 0; }

struct DevBuf {
    void *p = nullptr;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(uint64_t n) { return hipMalloc(&p, n ? n : 4); }
};

// alac_hip_decode_host / alac_hip_verify_host: the packets back to back and their offsets (prefix sum of the sizes) on the device
struct DevStream {
    DevBuf bytes, offs;
    uint64_t total = 0;     // stream bytes
    uint64_t pcmBytes = 0;  // of the decoded batch
};
int32_t upload_stream(alac_hip_ctx *ctx, const alac_hip_format &fmt, const uint8_t *h_stream, const uint32_t *h_packet_bytes,
                      uint32_t num_packets, DevStream &d)
{
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    d.pcmBytes = (uint64_t)num_packets * fmt.frame_size * fmt.num_channels * bytes_per_sample(fmt.bit_depth);
    std::vector<uint64_t> offs(num_packets + 1, 0);
    for (uint32_t i = 0; i < num_packets; i++) offs[i + 1] = offs[i] + h_packet_bytes[i];
    d.total = offs[num_packets];
    hipError_t e;
    if ((e = d.bytes.alloc(d.total + 16)) || (e = d.offs.alloc((num_packets + 1) * 8ull)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if ((e = hipMemcpyAsync(d.bytes.p, h_stream, d.total, hipMemcpyHostToDevice, ctx->stream)) ||
        (e = hipMemcpyAsync(d.offs.p, offs.data(), (num_packets + 1) * 8ull, hipMemcpyHostToDevice, ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    return ALAC_HIP_noErr;
}

// The host forms of the encode calls: the checks of the tables, the tables and the state staged to the device, `launch` (the
// device call on the staged buffers: (maxSeg, num samples, segment table, state, workspace, out, sizes, offsets) -> status),
// the results copied back.  wsBytes: the device call's workspace.
template <class Launch>
int32_t encode_host_common(alac_hip_ctx *ctx, const alac_hip_format *fmt, const uint32_t *h_num_samples, uint32_t num_packets,
                           const uint32_t *h_seg_first, uint32_t num_segments, int16_t *h_state, int32_t state_in,
                           uint8_t *h_out, uint64_t out_capacity, uint32_t *h_packet_bytes, uint64_t *out_total_bytes,
                           uint64_t wsBytes, Launch launch)
{
    const uint32_t np = num_packets, nseg = num_segments;
    const uint64_t stateBytes = (uint64_t)nseg * alac_hip_state_int16(fmt) * 2;
    const uint64_t outMax = alac_hip_encode_max_output_bytes(fmt, np);

    DevBuf dNs, dSeg, dState, dWs, dOut, dSizes, dOffs;
    hipError_t e;
    if ((e = dNs.alloc(np * 4ull)) || (e = dSeg.alloc((nseg + 1) * 4ull)) || (e = dState.alloc(stateBytes)) ||
        (e = dWs.alloc(wsBytes)) || (e = dOut.alloc(outMax)) || (e = dSizes.alloc(np * 4ull)) ||
        (e = dOffs.alloc((np + 1) * 8ull)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    hipStream_t st = ctx->stream;
    if ((e = hipMemcpyAsync(dNs.p, h_num_samples, np * 4ull, hipMemcpyHostToDevice, st)) ||
        (e = hipMemcpyAsync(dSeg.p, h_seg_first, (nseg + 1) * 4ull, hipMemcpyHostToDevice, st)))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    if (h_state && state_in)
        if ((e = hipMemcpyAsync(dState.p, h_state, stateBytes, hipMemcpyHostToDevice, st)))
            return fail(ctx, ALAC_HIP_ParamError, "H2D state", e);
    uint32_t maxSeg = 1;
    for (uint32_t s2 = 0; s2 < nseg; s2++) maxSeg = h_seg_first[s2 + 1] - h_seg_first[s2] > maxSeg ? h_seg_first[s2 + 1] - h_seg_first[s2] : maxSeg;
    int32_t rc = launch(maxSeg, (const uint32_t *)dNs.p, (const uint32_t *)dSeg.p, (int16_t *)dState.p,
                        (h_state && state_in) ? 1 : 0, dWs.p, (uint8_t *)dOut.p, outMax, (uint32_t *)dSizes.p,
                        (uint64_t *)dOffs.p);
    if (rc != ALAC_HIP_noErr) return rc;
    uint64_t total = 0;
    if ((e = hipMemcpyAsync(&total, (uint64_t *)dOffs.p + np, 8, hipMemcpyDeviceToHost, st)) ||
        (e = hipStreamSynchronize(st)))
        return fail(ctx, ALAC_HIP_ParamError, "encode execution", e);
    if (total > out_capacity) return fail(ctx, ALAC_HIP_MemFullError, "host output buffer too small");
    if ((e = hipMemcpyAsync(h_out, dOut.p, total, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h_packet_bytes, dSizes.p, np * 4ull, hipMemcpyDeviceToHost, st)))
        return fail(ctx, ALAC_HIP_ParamError, "D2H copy", e);
    if (h_state)
        if ((e = hipMemcpyAsync(h_state, dState.p, stateBytes, hipMemcpyDeviceToHost, st)))
            return fail(ctx, ALAC_HIP_ParamError, "D2H state", e);
    if ((e = hipStreamSynchronize(st))) return fail(ctx, ALAC_HIP_ParamError, "sync", e);
    if (int32_t hrc = check_handoff(ctx)) return hrc;
    if (out_total_bytes) *out_total_bytes = total;
    return ALAC_HIP_noErr;
}

// the checks of a host segment table every host form makes
int32_t host_segment_refusal(alac_hip_ctx *ctx, const uint32_t *h_seg_first, uint32_t num_segments, uint32_t num_packets)
{
    if (h_seg_first[0] != 0 || h_seg_first[num_segments] != num_packets)
        return fail(ctx, ALAC_HIP_ParamError, "segment table must start at 0 and end at num_packets");
    for (uint32_t s = 0; s < num_segments; s++)
        if (h_seg_first[s] > h_seg_first[s + 1]) return fail(ctx, ALAC_HIP_ParamError, "segment table not ascending");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    return ALAC_HIP_noErr;
}

}  // namespace

extern "C" {

int32_t alac_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return -1;
    return n;
}

int32_t alac_hip_create(alac_hip_ctx **out_ctx, int32_t device, void *stream)
{
    if (!out_ctx) return ALAC_HIP_ParamError;
    *out_ctx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return ALAC_HIP_ParamError;
    alac_hip_ctx *c = new (std::nothrow) alac_hip_ctx;
    if (!c) return ALAC_HIP_MemFullError;
    c->device = device;
    c->opt = alac_options_from_env();
    if (hipSetDevice(device) != hipSuccess) {
        delete c;
        return ALAC_HIP_ParamError;
    }
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            delete c;
            return ALAC_HIP_MemFullError;
        }
        c->ownStream = true;
    }
    if (hipHostMalloc((void **)&c->errHost, 64, hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&c->errDev, c->errHost, 0) != hipSuccess) {
        alac_hip_destroy(c);
        return ALAC_HIP_MemFullError;
    }
    c->errHost[0] = c->errHost[1] = 0;
    *out_ctx = c;
    return ALAC_HIP_noErr;
}

void alac_hip_destroy(alac_hip_ctx *ctx)
{
    if (!ctx) return;
    for (hipEvent_t e : ctx->events) (void)hipEventDestroy(e);
    ctx->events.clear();
    if (ctx->vsReady) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->vs.side[0]);
        (void)hipStreamDestroy(ctx->vs.side[0]);
        for (uint32_t i = 0; i < kSideEvents; i++) {
            (void)hipEventDestroy(ctx->vs.stagger[i]);
            (void)hipEventDestroy(ctx->vs.join[i]);
        }
        (void)hipEventDestroy(ctx->vs.fork);
    }
    if (ctx->mcReady) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->mcStream);
        (void)hipStreamDestroy(ctx->mcStream);
        (void)hipEventDestroy(ctx->mcFork);
        (void)hipEventDestroy(ctx->mcJoin);
    }
    if (ctx->ownStream && ctx->stream) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamDestroy(ctx->stream);
    }
    if (ctx->errHost) (void)hipHostFree(ctx->errHost);
    delete ctx;
}

int32_t alac_hip_synchronize(alac_hip_ctx *ctx)
{
    if (!ctx) return ALAC_HIP_ParamError;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipStreamSynchronize", e);
    return check_handoff(ctx);
}

int32_t alac_hip_set_option(alac_hip_ctx *ctx, const char *key, int32_t value)
{
    if (!ctx) return ALAC_HIP_ParamError;
    const AlacOptionKey *k = alac_option_find(key);
    if (!k) return fail(ctx, ALAC_HIP_ParamError, "unknown option");
    if (value < k->lo || value > k->hi) return fail(ctx, ALAC_HIP_ParamError, "option value outside its documented range");
    ctx->opt.*(k->slot) = value;
    return ALAC_HIP_noErr;
}

int32_t alac_hip_get_option(alac_hip_ctx *ctx, const char *key, int32_t *value)
{
    if (!ctx || !value) return ALAC_HIP_ParamError;
    const AlacOptionKey *k = alac_option_find(key);
    if (!k) return fail(ctx, ALAC_HIP_ParamError, "unknown option");
    *value = ctx->opt.*(k->slot);
    return ALAC_HIP_noErr;
}

uint64_t alac_hip_debug_waves_offset(const alac_hip_format *fmt, uint32_t num_packets, uint32_t num_segments)
{
    if (!format_ok(fmt) || fmt->num_channels > 2) return 0;
    return enc_layout(fmt, num_packets, num_segments ? num_segments : num_packets).rowReady;
}

const char *alac_hip_encode_regime(alac_hip_ctx *ctx, const alac_hip_format *fmt, uint32_t num_segments)
{
    if (!ctx || !format_ok(fmt)) return "";
    // the launcher's own plan (the longest segment only decides the overlap of chained positions, which the name leaves out)
    return v1_regime_name(v1_plan(fmt->num_channels, num_segments, 1, fmt->frame_size, ctx->opt).shape);
}

const char *alac_hip_last_error(const alac_hip_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void *alac_hip_stream(const alac_hip_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

uint64_t alac_hip_encode_workspace_bytes(const alac_hip_format *fmt, uint32_t num_packets, uint32_t num_segments)
{
    if (!format_ok(fmt)) return 0;
    if (fmt->num_channels > 2) return mc_layout(fmt, num_packets, num_segments ? num_segments : num_packets).total;
    return enc_layout(fmt, num_packets, num_segments ? num_segments : num_packets).total + lpc_table_bytes(num_packets);
}

uint32_t alac_hip_state_int16(const alac_hip_format *fmt)
{
    if (!format_ok(fmt)) return 0;
    McElement el[kMaxChannels];
    return ALAC_HIP_STATE_INT16 * (fmt->num_channels > 2 ? channel_elements(fmt->num_channels, el) : 1);
}

uint64_t alac_hip_encode_max_output_bytes(const alac_hip_format *fmt, uint32_t num_packets)
{
    if (!format_ok(fmt)) return 0;
    return max_output_bytes(fmt, num_packets);
}

// The refusals of alac_hip_encode_segmented that need no device work, in its order (the format is checked already); 0 when
// the call may go ahead.  alac_hip_encode_float runs them before it enqueues its conversion.
static int32_t encode_refusal(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_pcm, uint32_t num_packets,
                              const uint32_t *d_seg_first, uint32_t num_segments, const void *d_workspace,
                              uint64_t workspace_bytes, const uint8_t *d_out, uint64_t out_capacity,
                              const uint32_t *d_packet_bytes, const uint64_t *d_packet_offsets)
{
    const bool mc = fmt->num_channels > 2, lpc = ctx->opt.lpc != 0;
    if (mc && lpc) return fail(ctx, ALAC_HIP_ParamError, "option lpc: mono and stereo streams only");
    if (lpc) {
        if (ctx->opt.fastMode) return fail(ctx, ALAC_HIP_ParamError, "options lpc and fast_mode exclude each other");
        if ((uint64_t)fmt->frame_size * fmt->num_channels * 4 > 65536)
            return fail(ctx, ALAC_HIP_ParamError, "option lpc: frame_size x channels above 16 384");
        d_seg_first = nullptr;
    }
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!d_pcm || !d_workspace || !d_out || !d_packet_bytes || !d_packet_offsets)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (!d_seg_first) num_segments = num_packets;
    if (num_segments == 0 || num_segments > num_packets) return fail(ctx, ALAC_HIP_ParamError, "bad segment count");
    if (mc) {
        if (((uintptr_t)d_workspace & 255)) return fail(ctx, ALAC_HIP_ParamError, "misaligned workspace (256 B)");
        if ((uint64_t)num_packets * kMaxChannels > 0x7fffffffull) return fail(ctx, ALAC_HIP_ParamError, "too many packets");
        if (workspace_bytes < mc_layout(fmt, num_packets, num_segments).total)
            return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    } else {
        if (((uintptr_t)d_out & 3) || ((uintptr_t)d_workspace & 255) || ((uintptr_t)d_pcm & 15))
            return fail(ctx, ALAC_HIP_ParamError, "misaligned buffer (out 4 B, pcm 16 B, workspace 256 B)");
        if (workspace_bytes < enc_layout(fmt, num_packets, num_segments).total + (lpc ? lpc_table_bytes(num_packets) : 0))
            return fail(ctx, ALAC_HIP_ParamError, lpc ? "workspace too small (option lpc: size it for num_segments = num_packets)"
                                                      : "workspace too small");
    }
    if (out_capacity < max_output_bytes(fmt, num_packets))
        return fail(ctx, ALAC_HIP_ParamError, "output capacity below alac_hip_encode_max_output_bytes");
    return ALAC_HIP_noErr;
}

// the longest segment of a device segment table, read back (a host wait); refuses a table that is not ascending inside
// [0, num_packets]
static int32_t read_max_segment(alac_hip_ctx *ctx, const uint32_t *d_seg_first, uint32_t num_segments, uint32_t num_packets,
                                uint32_t &maxSeg)
{
    std::vector<uint32_t> sf(num_segments + 1);
    if (hipMemcpyAsync(sf.data(), d_seg_first, (num_segments + 1) * 4ull, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return fail(ctx, ALAC_HIP_ParamError, "reading d_seg_first");
    maxSeg = 0;
    for (uint32_t s = 0; s < num_segments; s++) {
        if (sf[s + 1] < sf[s] || sf[s + 1] > num_packets) return fail(ctx, ALAC_HIP_ParamError, "bad d_seg_first");
        maxSeg = sf[s + 1] - sf[s] > maxSeg ? sf[s + 1] - sf[s] : maxSeg;
    }
    return ALAC_HIP_noErr;
}

static int32_t encode_elements(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_pcm,
                               const uint32_t *d_num_samples, uint32_t num_packets, const uint32_t *d_seg_first,
                               uint32_t num_segments, int16_t *d_state, int32_t state_in, void *d_workspace,
                               uint64_t workspace_bytes, uint8_t *d_out, uint64_t out_capacity,
                               uint32_t *d_packet_bytes, uint64_t *d_packet_offsets, uint32_t maxSegHint);

// one mono / stereo batch; `timed` = this call may consume a slot of the armed stage timing
static int32_t encode_core(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_pcm,
                           const uint32_t *d_num_samples, uint32_t num_packets, const uint32_t *d_seg_first,
                           uint32_t num_segments, int16_t *d_state, int32_t state_in, void *d_workspace,
                           uint64_t workspace_bytes, uint8_t *d_out, uint64_t out_capacity,
                           uint32_t *d_packet_bytes, uint64_t *d_packet_offsets, bool timed, uint32_t maxSegHint);

int32_t alac_hip_encode_segmented(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_pcm,
                                  const uint32_t *d_num_samples, uint32_t num_packets, const uint32_t *d_seg_first,
                                  uint32_t num_segments, uint32_t max_segment_packets, int16_t *d_state, int32_t state_in,
                                  void *d_workspace, uint64_t workspace_bytes, uint8_t *d_out, uint64_t out_capacity,
                                  uint32_t *d_packet_bytes, uint64_t *d_packet_offsets)
{
    if (!ctx) return ALAC_HIP_ParamError;
    if (!format_ok(fmt)) return fail(ctx, ALAC_HIP_ParamError, "unsupported format");
    if (fmt->num_channels > 2)
        return encode_elements(ctx, fmt, d_pcm, d_num_samples, num_packets, d_seg_first, num_segments, d_state, state_in,
                               d_workspace, workspace_bytes, d_out, out_capacity, d_packet_bytes, d_packet_offsets,
                               max_segment_packets);
    return encode_core(ctx, fmt, d_pcm, d_num_samples, num_packets, d_seg_first, num_segments, d_state, state_in,
                       d_workspace, workspace_bytes, d_out, out_capacity, d_packet_bytes, d_packet_offsets, true,
                       max_segment_packets);
}

int32_t alac_hip_encode(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_pcm,
                        const uint32_t *d_num_samples, uint32_t num_packets, const uint32_t *d_seg_first,
                        uint32_t num_segments, int16_t *d_state, int32_t state_in, void *d_workspace,
                        uint64_t workspace_bytes, uint8_t *d_out, uint64_t out_capacity,
                        uint32_t *d_packet_bytes, uint64_t *d_packet_offsets)
{
    return alac_hip_encode_segmented(ctx, fmt, d_pcm, d_num_samples, num_packets, d_seg_first, num_segments, 0, d_state, state_in,
                                     d_workspace, workspace_bytes, d_out, out_capacity, d_packet_bytes, d_packet_offsets);
}

// ---- float32 input: quantize into a stage at the end of the workspace, then alac_hip_encode_segmented on it -------------
// the staged integer PCM of a batch (+ 64: slack behind the last packet, like the gathered copies of a > 2-channel batch)
static uint64_t float_stage_bytes(const alac_hip_format *fmt, uint32_t num_packets)
{
    return align_up((uint64_t)num_packets * fmt->frame_size * fmt->num_channels * bytes_per_sample(fmt->bit_depth) + 64, 256);
}

uint64_t alac_hip_encode_float_workspace_bytes(const alac_hip_format *fmt, uint32_t num_packets, uint32_t num_segments)
{
    if (!format_ok(fmt)) return 0;
    return align_up(alac_hip_encode_workspace_bytes(fmt, num_packets, num_segments), 256) + float_stage_bytes(fmt, num_packets);
}

int32_t alac_hip_encode_float(alac_hip_ctx *ctx, const alac_hip_format *fmt, const float *d_in, uint64_t channel_stride,
                              uint64_t frame_stride, const uint32_t *d_num_samples, uint32_t num_packets,
                              const uint32_t *d_seg_first, uint32_t num_segments, uint32_t max_segment_packets,
                              int16_t *d_state, int32_t state_in, void *d_workspace, uint64_t workspace_bytes, uint8_t *d_out,
                              uint64_t out_capacity, uint32_t *d_packet_bytes, uint64_t *d_packet_offsets,
                              uint32_t *d_clipped)
{
    if (!ctx) return ALAC_HIP_ParamError;
    if (!format_ok(fmt)) return fail(ctx, ALAC_HIP_ParamError, "unsupported format");
    if (num_packets == 0)
        return encode_refusal(ctx, fmt, nullptr, 0, d_seg_first, num_segments, d_workspace, workspace_bytes, d_out,
                              out_capacity, d_packet_bytes, d_packet_offsets);
    const uint32_t C = fmt->num_channels;
    if (!d_in) return fail(ctx, ALAC_HIP_ParamError, "null d_in");
    if ((uintptr_t)d_in & 3) return fail(ctx, ALAC_HIP_ParamError, "misaligned d_in (4 B)");
    if (frame_stride == 0) return fail(ctx, ALAC_HIP_ParamError, "frame_stride 0");
    if (channel_stride == 0 && C > 1) return fail(ctx, ALAC_HIP_ParamError, "channel_stride 0 with more than one channel");
    // the largest index the conversion can form, and its byte offset: (C - 1) * channel_stride + (frames - 1) * frame_stride
    uint64_t rows, cols, last;
    if (__builtin_mul_overflow((uint64_t)(C - 1), channel_stride, &rows) ||
        __builtin_mul_overflow((uint64_t)num_packets * fmt->frame_size - 1, frame_stride, &cols) ||
        __builtin_add_overflow(rows, cols, &last) || last > UINT64_MAX / sizeof(float))
        return fail(ctx, ALAC_HIP_ParamError, "the largest index into d_in overflows 64 bits");
    // the stage: the last whole 256-byte blocks of the workspace; the encoder gets everything in front of it
    const uint64_t stage = float_stage_bytes(fmt, num_packets);
    if (workspace_bytes < stage) return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    const uint64_t encBytes = (workspace_bytes - stage) & ~255ull;
    uint8_t *pcm = d_workspace ? (uint8_t *)d_workspace + encBytes : nullptr;
    if (int32_t rc = encode_refusal(ctx, fmt, pcm, num_packets, d_seg_first, num_segments, d_workspace, encBytes, d_out,
                                    out_capacity, d_packet_bytes, d_packet_offsets))
        return rc;
    // the encoder's own read-back of a segment table without a bound (tap-parallel path) may refuse it: run that check before
    // anything is enqueued (the encoder reads the table again)
    if (d_seg_first && !max_segment_packets && C <= 2 && !ctx->opt.lpc && !use_lane_encoder(ctx)) {
        uint32_t maxSeg = 0;
        if (int32_t rc = read_max_segment(ctx, d_seg_first, num_segments, num_packets, maxSeg)) return rc;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    FloatInArgs a;
    a.in = d_in;
    a.channelStride = channel_stride;
    a.frameStride = frame_stride;
    a.numSamples = d_num_samples;
    a.numPackets = num_packets;
    a.frameSize = fmt->frame_size;
    a.channels = C;
    a.pcm = pcm;
    a.clipped = d_clipped;
    const hipError_t e = launch_float_to_pcm(fmt->bit_depth, a, ctx->stream);
    if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "float conversion launch", e);
    return alac_hip_encode_segmented(ctx, fmt, pcm, d_num_samples, num_packets, d_seg_first, num_segments, max_segment_packets,
                                     d_state, state_in, d_workspace, encBytes, d_out, out_capacity, d_packet_bytes,
                                     d_packet_offsets);
}

static int32_t encode_elements(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_pcm,
                               const uint32_t *d_num_samples, uint32_t num_packets, const uint32_t *d_seg_first,
                               uint32_t num_segments, int16_t *d_state, int32_t state_in, void *d_workspace,
                               uint64_t workspace_bytes, uint8_t *d_out, uint64_t out_capacity,
                               uint32_t *d_packet_bytes, uint64_t *d_packet_offsets, uint32_t maxSegHint)
{
    if (int32_t rc = encode_refusal(ctx, fmt, d_pcm, num_packets, d_seg_first, num_segments, d_workspace, workspace_bytes,
                                    d_out, out_capacity, d_packet_bytes, d_packet_offsets))
        return rc;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!d_seg_first) num_segments = num_packets;
    const McLayout M = mc_layout(fmt, num_packets, num_segments);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    uint8_t *ws = (uint8_t *)d_workspace;
    const uint32_t bps = bytes_per_sample(fmt->bit_depth);
    hipStream_t mainStream = ctx->stream;

    // the stereo batch runs on the context's stream, the mono batch beside it on a second stream (both are bound by
    // the latency of one wave, not by the machine)
    const bool both = M.g[0].count && M.g[1].count;
    bool side = both;
    if (side && !ensure_second_stream(ctx)) return fail(ctx, ALAC_HIP_MemFullError, "creating the second stream");
    if (side) {
        (void)hipEventRecord(ctx->mcFork, mainStream);
        (void)hipStreamWaitEvent(ctx->mcStream, ctx->mcFork, 0);
    }
    int32_t rc = ALAC_HIP_noErr;
    hipError_t copyErr = hipSuccess;
    // SetFastMode is consulted for 2-channel STREAMS only (codec/ALACEncoder.cu:998-1001): the stereo elements of a
    // > 2-channel stream are searched like everything else
    const int32_t fastModeOfCtx = ctx->opt.fastMode;
    ctx->opt.fastMode = 0;
    struct Restore {
        alac_hip_ctx *c;
        int32_t v;
        ~Restore() { c->opt.fastMode = v; }
    } restoreFast{ctx, fastModeOfCtx};
    for (int gi = 0; gi < 2 && rc == ALAC_HIP_noErr; gi++) {
        const McGroup &G = M.g[gi];
        if (!G.count) continue;
        hipStream_t st = (side && gi == 1) ? ctx->mcStream : mainStream;
        const alac_hip_format gf = element_format(fmt, G.channels);
        const uint64_t elemPcm = (uint64_t)num_packets * fmt->frame_size * G.channels * bps;
        for (uint32_t k = 0; k < G.count; k++)
            launch_mc_gather((const uint8_t *)d_pcm, ws + G.gather + k * elemPcm, d_num_samples, num_packets, fmt->frame_size,
                             fmt->num_channels, M.el[G.elem[k]].first, G.channels, bps, st);
        uint32_t *ns = d_num_samples ? (uint32_t *)(ws + G.ns) : nullptr;
        uint32_t *seg = d_seg_first ? (uint32_t *)(ws + G.seg) : nullptr;
        launch_mc_tables(d_num_samples, num_packets, d_seg_first, num_segments, G.count, ns, seg, st);
        // coefficient rows: the caller's [element][segment][64] <-> the batch's [k][segment][64]
        int16_t *gstate = d_state ? (int16_t *)(ws + G.state) : nullptr;
        const uint64_t rowBytes = (uint64_t)num_segments * ALAC_HIP_STATE_INT16 * 2;
        if (gstate && state_in)
            for (uint32_t k = 0; k < G.count && copyErr == hipSuccess; k++)
                copyErr = hipMemcpyAsync((uint8_t *)gstate + k * rowBytes, (const uint8_t *)d_state + G.elem[k] * rowBytes,
                                         rowBytes, hipMemcpyDeviceToDevice, st);
        ctx->stream = st;
        rc = encode_core(ctx, &gf, ws + G.gather, ns, G.count * num_packets, seg, G.count * num_segments, gstate, state_in,
                         ws + G.sub, G.subBytes, ws + G.out, G.outCap, (uint32_t *)(ws + G.sizes), (uint64_t *)(ws + G.offs),
                         false, maxSegHint);
        ctx->stream = mainStream;
        if (gstate && rc == ALAC_HIP_noErr)
            for (uint32_t k = 0; k < G.count && copyErr == hipSuccess; k++)
                copyErr = hipMemcpyAsync((uint8_t *)d_state + G.elem[k] * rowBytes, (const uint8_t *)gstate + k * rowBytes,
                                         rowBytes, hipMemcpyDeviceToDevice, st);
    }
    if (side) {
        (void)hipEventRecord(ctx->mcJoin, ctx->mcStream);
        (void)hipStreamWaitEvent(mainStream, ctx->mcJoin, 0);
    }
    // (the second stream is joined above whatever happened, so the context's stream stays the only one to wait on)
    if (rc != ALAC_HIP_noErr) return rc;
    if (copyErr != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "coefficient state copy", copyErr);
    McSpliceArgs sa;
    sa.numElements = M.numElements;
    sa.numPackets = num_packets;
    for (uint32_t e = 0; e < M.numElements; e++) {
        const McGroup &G = M.g[M.groupOf[e]];
        sa.el[e] = M.el[e];
        sa.src[e] = ws + G.out;
        sa.srcOffsets[e] = (const uint64_t *)(ws + G.offs) + (uint64_t)M.indexInGroup[e] * num_packets;
    }
    sa.elemBits = (uint32_t *)(ws + M.elemBits);
    sa.packetBytes = d_packet_bytes;
    sa.offsets = d_packet_offsets;
    sa.out = d_out;
    launch_mc_splice(sa, mainStream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "splice launch", e);
    return ALAC_HIP_noErr;
}

// the argument block of the tap-parallel pipeline: the batch of `ea`, its scratch in the workspace `ws` laid out by L, the
// switches of plan P; stateInternal: the coefficient rows live in the workspace (no caller state)
static V1Args v1_args(const alac_hip_ctx *ctx, const EncodeArgs &ea, const EncLayout &L, uint8_t *ws, const V1Plan &P,
                      bool stateInternal)
{
    V1Args A{};  // (flags2, thru and narrow, which no kernel reads, stay 0)
    A.S = {ea.pcm, ea.numSamples, ea.segFirst, ea.numSegments, ea.frameSize, 0, 0, ea.numSegments, ea.numPackets, ea.segMax};
    A.state = stateInternal ? (int16_t *)(ws + L.state) : ea.state;
    A.recs = ea.recs;
    A.resA = (int32_t *)(ws + L.resA);
    A.resB = (int32_t *)(ws + L.resB);
    A.resC = (int32_t *)(ws + L.resC);
    A.bits1 = (uint32_t *)(ws + L.bits1);
    A.cost2 = (uint32_t *)(ws + L.cost2);
    A.chainsPad = L.chainsPad;
    A.bitWords = ea.bitWords;
    A.wcap = ea.wcap;
    A.dumpSlot = ea.numPackets * 2;
    A.packetBytes = ea.packetBytes;
    // progress words: the search launch's, then the final launch's (overlapped positions of a chained batch run side by side)
    A.flags = (uint32_t *)(ws + L.flags);
    A.flagsF = A.ovFlagsF = A.flags + (L.chainsPad / 8 + 16);
    A.ovRowReady = (uint32_t *)(ws + L.rowReady);
    A.dbg = ctx->opt.debugWaves ? A.ovRowReady : nullptr;  // (the row-ready words are only used by chained tiny batches)
    // rows that live in the workspace and hold no caller state are never read before they are written: the kernels of the first
    // packet position take init_coefs as constants (load_row) instead of a k_init_state launch writing them first — except
    // in fast mode, where no search launch takes them as constants
    A.virgin = stateInternal && !P.fast ? 1u : 0u;
    A.foldDecide = P.shape == V1Shape::Latency ? 1u : 0u;
    // pubMask 0: producers publish after every tile, rows written through (a release fence per publish cost ~11 us)
    A.idleFast = P.shape == V1Shape::Throughput ? 0u : 1u;
    A.ho = handoff_ctl(ctx);
    A.cls = (ClassInfo *)(ws + L.cls);
    A.colChain = (uint32_t *)(ws + L.colChain);
    A.colsPad = L.colsPad;
    // the second wave first walks [0, splitAt) keeping only the coder's state (~half the instructions of coding), then codes
    // the rest: both waves finish together at ~2/3 of the frame
    A.bitWordsB = P.split ? (uint32_t *)(ws + L.bitWordsB) : nullptr;
    A.bitsB = L.bitsB ? (uint32_t *)(ws + L.bitsB) : nullptr;
    A.splitAt = v1_split_at(ea.frameSize);
    return A;
}

static int32_t encode_core(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_pcm,
                           const uint32_t *d_num_samples, uint32_t num_packets, const uint32_t *d_seg_first,
                           uint32_t num_segments, int16_t *d_state, int32_t state_in, void *d_workspace,
                           uint64_t workspace_bytes, uint8_t *d_out, uint64_t out_capacity,
                           uint32_t *d_packet_bytes, uint64_t *d_packet_offsets, bool timed, uint32_t maxSegHint)
{
    // LPC mode: every packet is its own segment, whatever table the caller passes; the coefficient state is neither read
    // nor written
    if (int32_t rc = encode_refusal(ctx, fmt, d_pcm, num_packets, d_seg_first, num_segments, d_workspace, workspace_bytes,
                                    d_out, out_capacity, d_packet_bytes, d_packet_offsets))
        return rc;
    const bool lpc = ctx->opt.lpc != 0;
    if (lpc) {
        d_seg_first = nullptr;
        d_state = nullptr;
        state_in = 0;
        maxSegHint = 0;
    }
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!d_seg_first) num_segments = num_packets;
    const EncLayout L = enc_layout(fmt, num_packets, num_segments);

    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    uint8_t *ws = (uint8_t *)d_workspace;
    EncodeArgs ea;
    ea.pcm = (const uint8_t *)d_pcm;
    ea.numSamples = d_num_samples;
    ea.segFirst = d_seg_first;
    ea.numSegments = num_segments;
    ea.frameSize = fmt->frame_size;
    ea.state = d_state;
    ea.stateIn = state_in;
    ea.pred = (int32_t *)(ws + L.pred);
    ea.predStride = L.predStride;
    ea.bitWords = (uint32_t *)(ws + L.bitWords);
    ea.wcap = L.wcap;
    ea.recs = (PacketRec *)(ws + L.recs);
    ea.packetBytes = d_packet_bytes;
    // a table with the caller's bound (alac_hip_encode_segmented) is not read back: the kernels test every entry they use
    const bool unread = d_seg_first && maxSegHint;
    ea.numPackets = num_packets;
    ea.segMax = unread ? (maxSegHint < num_packets ? maxSegHint : num_packets) : 0xffffffffu;
    ea.segBad = unread ? (uint32_t *)(ws + L.segBad) : nullptr;
    PackArgs pa;
    pa.pcm = ea.pcm;
    pa.recs = ea.recs;
    pa.bitWords = ea.bitWords;
    pa.wcap = L.wcap;
    pa.frameSize = fmt->frame_size;
    pa.offsets = d_packet_offsets;
    pa.out = d_out;
    pa.segBad = ea.segBad;
    constexpr uint32_t EV = kEventBlocks * (kNumStages + 1);
    hipEvent_t *ev = nullptr;
    if (timed && ctx->profile && (uint64_t)(ctx->profCalls + 1) * EV <= ctx->events.size())
        ev = &ctx->events[ctx->profCalls++ * EV];
    hipError_t e;
    // the caller's bound on the segment length (alac_hip_encode_segmented) is checked on the device whatever kernels run
    if (unread)
        launch_check_segments(d_seg_first, num_segments, num_packets, ea.segMax, ctx->errDev ? ctx->errDev + 1 : nullptr,
                              ea.segBad, ctx->stream);
    if (ev) ctx->profLane.push_back(use_lane_encoder(ctx));
    if (use_lane_encoder(ctx)) {
        e = launch_encode(fmt->bit_depth, fmt->num_channels, ea, pa, num_packets, ctx->stream,
                          ev ? ev + (kNumStages + 1) : nullptr);
    } else {
        if (!ctx->vsReady) {
            bool ok = hipEventCreateWithFlags(&ctx->vs.fork, hipEventDisableTiming) == hipSuccess &&
                      hipStreamCreateWithFlags(&ctx->vs.side[0], hipStreamNonBlocking) == hipSuccess;
            for (uint32_t i = 0; ok && i < kSideEvents; i++)
                ok = hipEventCreateWithFlags(&ctx->vs.stagger[i], hipEventDisableTiming) == hipSuccess &&
                     hipEventCreateWithFlags(&ctx->vs.join[i], hipEventDisableTiming) == hipSuccess;
            if (!ok) return fail(ctx, ALAC_HIP_MemFullError, "creating side streams");
            ctx->vsReady = true;
        }
        // packets per segment: the pipeline runs once per packet position (a chained segment is serial)
        uint32_t maxSeg = 1;
        if (d_seg_first && maxSegHint) {
            // the caller knows how long its longest segment is (alac_hip_encode_segmented): no read-back of the table, no
            // host wait.  The bound is checked on the device; a table that contradicts it fails the next synchronize.
            maxSeg = maxSegHint < num_packets ? maxSegHint : num_packets;
        } else if (d_seg_first) {
            if (int32_t rc = read_max_segment(ctx, d_seg_first, num_segments, num_packets, maxSeg)) return rc;
        }
        const V1Plan P = v1_plan(fmt->num_channels, num_segments, maxSeg, fmt->frame_size, ctx->opt);
        const V1Args A = v1_args(ctx, ea, L, ws, P, d_state == nullptr);
        // rows that hold no caller state and are not taken as constants (V1Args::virgin) get init_coefs first
        const bool initState = !(d_state && state_in) && !A.virgin;
        e = launch_encode_v1(fmt->bit_depth, fmt->num_channels, A, P, initState, pa, ctx->vs, num_packets, maxSeg, ctx->stream, ev);
    }
    if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "encode launch", e);
    if (lpc) {
        // Apple's independent packets are in the records and bit strings: the LPC candidates replace channels they beat,
        // then the sizes are scanned and the packets packed again, with the LPC headers
        LpcArgs la;
        la.pcm = ea.pcm;
        la.frameSize = fmt->frame_size;
        la.recs = ea.recs;
        la.packetBytes = d_packet_bytes;
        la.bitWords = ea.bitWords;
        la.wcap = L.wcap;
        la.lpc = (LpcChan *)(ws + L.total);
        e = launch_lpc(fmt->bit_depth, fmt->num_channels, la, num_packets, ctx->stream);
        if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "lpc launch", e);
        pa.lpc = la.lpc;
        launch_scan_pack(fmt->bit_depth, fmt->num_channels, d_packet_bytes, pa, num_packets, ctx->stream, nullptr);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "lpc pack launch", e);
    }
    return ALAC_HIP_noErr;
}

uint32_t alac_hip_num_stages(void) { return kNumStages; }

const char *alac_hip_stage_name(uint32_t stage)
{
    static const char *names[kNumStages] = {"lms_search1", "golomb_count1", "lms_search2", "golomb_count2",
                                            "lms_final",   "golomb_final",  "finalize_scan", "pack"};
    return stage < kNumStages ? names[stage] : "";
}

int32_t alac_hip_profile_begin(alac_hip_ctx *ctx, uint32_t max_calls)
{
    if (!ctx) return ALAC_HIP_ParamError;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    while (ctx->events.size() < (size_t)max_calls * kEventBlocks * (kNumStages + 1)) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return fail(ctx, ALAC_HIP_MemFullError, "hipEventCreate");
        ctx->events.push_back(e);
    }
    ctx->profCalls = 0;
    ctx->profLane.clear();
    ctx->profile = max_calls != 0;
    return ALAC_HIP_noErr;
}

int32_t alac_hip_profile_end(alac_hip_ctx *ctx, uint32_t *out_calls, float *out_stage_ms, uint32_t *out_launches)
{
    if (!ctx) return ALAC_HIP_ParamError;
    ctx->profile = false;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipStreamSynchronize", e);
    constexpr uint32_t BLK = kNumStages + 1;
    constexpr uint32_t EV = kEventBlocks * BLK;
    double t[kNumStages] = {0};
    double launches[kNumStages] = {0};
    auto elapsed = [&](hipEvent_t a, hipEvent_t b, double &acc) -> bool {
        float ms = 0;
        if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return false;
        acc += ms;
        return true;
    };
    for (uint32_t c = 0; c < ctx->profCalls; c++) {
        // block 0: the predictor / Golomb stages of the tap-parallel pipeline; block 1: finalize, scan, pack — and every
        // stage of the lane encoder
        hipEvent_t *base = &ctx->events[(size_t)c * EV];
        for (uint32_t k = 0; k < kNumStages; k++) {
            hipEvent_t *blk = (ctx->profLane[c] || k >= kStageScan) ? base + BLK : base;
            if (!elapsed(blk[k], blk[k + 1], t[k])) return fail(ctx, ALAC_HIP_ParamError, "hipEventElapsedTime");
            launches[k] += 1;
        }
    }
    if (out_calls) *out_calls = ctx->profCalls;
    const double n = ctx->profCalls ? ctx->profCalls : 1;
    for (uint32_t k = 0; k < kNumStages; k++) {
        if (out_stage_ms) out_stage_ms[k] = launches[k] > 0 ? (float)(t[k] / launches[k]) : 0.0f;  // per launch
        if (out_launches) out_launches[k] = (uint32_t)(launches[k] / n + 0.5);                   // per call
    }
    return ALAC_HIP_noErr;
}

uint32_t alac_hip_magic_cookie(const alac_hip_format *fmt, uint32_t max_frame_bytes, uint32_t avg_bit_rate,
                               uint8_t *c)
{
    if (!format_ok(fmt) || !c) return 0;
    auto be32 = [](uint8_t *p, uint32_t v) {
        p[0] = (uint8_t)(v >> 24);
        p[1] = (uint8_t)(v >> 16);
        p[2] = (uint8_t)(v >> 8);
        p[3] = (uint8_t)v;
    };
    be32(c + 0, fmt->frame_size);
    c[4] = 0;  // kALACCompatibleVersion
    c[5] = (uint8_t)fmt->bit_depth;
    c[6] = (uint8_t)kPB0;
    c[7] = (uint8_t)kMB0;
    c[8] = (uint8_t)kKB0;
    c[9] = (uint8_t)fmt->num_channels;
    c[10] = 0;
    c[11] = 255;  // MAX_RUN_DEFAULT
    be32(c + 12, max_frame_bytes);
    be32(c + 16, avg_bit_rate);
    be32(c + 20, fmt->sample_rate);
    return 24;
}

uint32_t alac_hip_magic_cookie_size(const alac_hip_format *fmt)
{
    if (!format_ok(fmt)) return 0;
    return fmt->num_channels > 2 ? 48 : 24;  // + kChannelAtomSize 12 + sizeof(ALACAudioChannelLayout) 12
}

uint32_t alac_hip_magic_cookie_full(const alac_hip_format *fmt, uint32_t max_frame_bytes, uint32_t avg_bit_rate,
                                    uint8_t *c, uint32_t capacity)
{
    const uint32_t need = alac_hip_magic_cookie_size(fmt);
    if (!need || !c || capacity < need) return 0;  // "no incomplete cookies", codec/ALACEncoder.cu:1136-1139
    alac_hip_magic_cookie(fmt, max_frame_bytes, avg_bit_rate, c);
    if (need == 24) return 24;
    // ALACChannelLayoutTags, codec/ALACAudioTypes.h:103-124
    static const uint32_t tags[kMaxChannels] = {(100u << 16) | 1, (101u << 16) | 2, (113u << 16) | 3, (116u << 16) | 4,
                                                (120u << 16) | 5, (124u << 16) | 6, (142u << 16) | 7, (127u << 16) | 8};
    memset(c + 24, 0, 24);
    c[27] = 24;  // theChannelAtom[3] = sizeof(ALACAudioChannelLayout) + kChannelAtomSize
    memcpy(c + 28, "chan", 4);
    // the fork stores mChannelLayoutTag in host byte order (:1120 has no Swap32NtoB): little endian
    const uint32_t t = tags[fmt->num_channels - 1];
    c[36] = (uint8_t)t;
    c[37] = (uint8_t)(t >> 8);
    c[38] = (uint8_t)(t >> 16);
    c[39] = (uint8_t)(t >> 24);
    return 48;
}

int32_t alac_hip_format_from_cookie(const uint8_t *ck, uint32_t size, alac_hip_format *out)
{
    if (!ck || !out) return ALAC_HIP_ParamError;
    ck = cookie_config(ck, size);
    if (size < 24) return ALAC_HIP_ParamError;
    if (ck[4] > 0) return ALAC_HIP_ParamError;  // compatibleVersion <= kALACVersion (:153)
    out->frame_size = ((uint32_t)ck[0] << 24) | ((uint32_t)ck[1] << 16) | ((uint32_t)ck[2] << 8) | ck[3];
    out->bit_depth = ck[5];
    out->num_channels = ck[9];
    out->sample_rate = ((uint32_t)ck[20] << 24) | ((uint32_t)ck[21] << 16) | ((uint32_t)ck[22] << 8) | ck[23];
    return ALAC_HIP_noErr;
}

uint64_t alac_hip_decode_workspace_bytes(const alac_hip_format *fmt, uint32_t num_packets)
{
    if (!format_ok(fmt)) return 0;
    return dec_layout(fmt, num_packets).total;
}

uint64_t alac_hip_decode_workspace_bytes_stream(const alac_hip_format *fmt, uint32_t num_packets, uint64_t stream_bytes)
{
    if (!format_ok(fmt)) return 0;
    return dec_layout(fmt, num_packets, stream_bytes).total;
}

}  // extern "C"

namespace {
int32_t cookie_format(alac_hip_ctx *ctx, const uint8_t *cookie, uint32_t size, alac_hip_format &fmt)
{
    if (alac_hip_format_from_cookie(cookie, size, &fmt) != ALAC_HIP_noErr) return fail(ctx, ALAC_HIP_ParamError, "bad magic cookie");
    if (!format_ok(&fmt)) return fail(ctx, ALAC_HIP_ParamError, "unsupported format in cookie");
    return ALAC_HIP_noErr;
}

// alac_hip_decode (kPcmStore), alac_hip_verify's decode pass (kPcmVerify: d_pcm_out is the expected PCM, only read, and
// verifyMismatch the first-mismatch words) and alac_hip_decode_float (kPcmFloat: d_pcm_out is planar float32, channel rows
// channelStride floats apart)
int32_t decode_impl(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *d_stream,
                    const uint64_t *d_packet_offsets, uint32_t num_packets, void *d_workspace, uint64_t workspace_bytes,
                    uint8_t *d_pcm_out, uint32_t *d_num_samples_out, int32_t *d_status, PcmMode mode,
                    uint32_t *verifyMismatch = nullptr, uint64_t channelStride = 0)
{
    if (!ctx) return ALAC_HIP_ParamError;
    alac_hip_format fmt;
    if (int32_t rc = cookie_format(ctx, h_cookie, cookie_size, fmt)) return rc;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!d_stream || !d_packet_offsets || !d_workspace || !d_pcm_out || !d_num_samples_out || !d_status)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (((uintptr_t)d_workspace & 255) || ((uintptr_t)d_pcm_out & 3))
        return fail(ctx, ALAC_HIP_ParamError, "misaligned buffer");
    DecLayout L = dec_layout(&fmt, num_packets);
    if (workspace_bytes < L.total) return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    L.capWords = (workspace_bytes - L.words) / 4;  // all of it: packets that do not fit the staged words get status -50
    uint32_t size = cookie_size;
    const uint8_t *ck = cookie_config(h_cookie, size);  // pb / mb / kb
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    uint8_t *ws = (uint8_t *)d_workspace;
    DecodeArgs da;
    da.stream = d_stream;
    da.offsets = d_packet_offsets;
    da.numPackets = num_packets;
    da.frameSize = fmt.frame_size;
    da.bitDepth = fmt.bit_depth;
    da.numChannels = fmt.num_channels;
    da.pb = ck[6];
    da.mb = ck[7];
    da.kb = ck[8];
    // Local hardening, NOT reference behaviour (codec/ag_dec.c:282-286 only checks its pointers; ALACDecoder::Init takes any
    // pb / mb / kb): the kernels shift by kb (k = min(lg3a, kb), m = (1 << k) - 1), so kb outside 1..16 would be an undefined
    // or zero-width shift, and pb = 0 freezes the mean at values the quotient code does not expect.  No encoder writes either.
    if (da.kb < 1 || da.kb > 16 || da.pb == 0) return fail(ctx, ALAC_HIP_ParamError, "bad AG parameters in cookie (pb / kb)");
    da.maxElems = L.maxElems;
    da.recs = (DecRec *)(ws + L.recs);
    da.resid = (int32_t *)(ws + L.resid);
    da.pcmOut = d_pcm_out;
    da.numSamplesOut = d_num_samples_out;
    da.statusOut = d_status;
    da.ho = handoff_ctl(ctx);
    da.optFused = ctx->opt.decFused;
    da.optPair = ctx->opt.decPair;
    da.optDirect = ctx->opt.decDirect;
    da.pcmMode = mode;
    if (mode == kPcmVerify) da.firstMismatch = verifyMismatch;
    if (mode == kPcmFloat) da.channelStride = channelStride;
    da.frameBytes = fmt.num_channels * bytes_per_sample(fmt.bit_depth);
    hipError_t e;
    if (use_lane_decoder(ctx)) {
        e = launch_decode(da, ctx->stream);
    } else if (fmt.num_channels > 2) {
        // one pass per element of the channel count's sequence (the position of element k + 1 is only known once
        // element k is entropy-decoded); a stream with another sequence is decoded again by the lane decoder, which
        // follows whatever the packets carry.  This is the one place where the call waits for the GPU.
        McElement el[kMaxChannels];
        const uint32_t nel = channel_elements(fmt.num_channels, el);
        e = launch_decode_v1_elements(da, el, nel, (uint32_t *)(ws + L.words), L.capWords, da.resid, (uint32_t *)(ws + L.prog),
                                      (uint32_t *)(ws + L.elemBit), (uint32_t *)(ws + L.mismatch), ctx->stream);
        uint32_t mismatch = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&mismatch, ws + L.mismatch, 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess && mismatch) e = launch_decode(da, ctx->stream);
    } else {
        // A mono / stereo stream whose packets carry another element sequence (two SCEs for two channels, fill in
        // front of ...: status -4 from the fast pipeline, counted by its header kernel) is decoded again by the lane decoder,
        // which follows whatever the packets carry.  No host round trip: its kernels are gated on that device-side count.
        e = launch_decode_v1(da, (uint32_t *)(ws + L.words), L.capWords, da.resid, (uint32_t *)(ws + L.prog), ctx->stream,
                             (uint32_t *)(ws + L.mismatch));
        if (e == hipSuccess) {
            DecodeArgs dg = da;
            dg.gate = (const uint32_t *)(ws + L.mismatch);
            e = launch_decode(dg, ctx->stream);
        }
    }
    if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "decode launch", e);
    return ALAC_HIP_noErr;
}
}  // namespace

extern "C" {

int32_t alac_hip_decode(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *d_stream,
                        const uint64_t *d_packet_offsets, uint32_t num_packets, void *d_workspace,
                        uint64_t workspace_bytes, uint8_t *d_pcm_out, uint32_t *d_num_samples_out,
                        int32_t *d_status)
{
    return decode_impl(ctx, h_cookie, cookie_size, d_stream, d_packet_offsets, num_packets, d_workspace, workspace_bytes,
                       d_pcm_out, d_num_samples_out, d_status, kPcmStore);
}

// ---- decode to planar float32: alac_hip_decode with the PCM store sites writing scaled floats ----------------------------
int32_t alac_hip_decode_float(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *d_stream,
                              const uint64_t *d_packet_offsets, uint32_t num_packets, void *d_workspace,
                              uint64_t workspace_bytes, float *d_out, uint64_t channel_stride, uint32_t *d_num_samples_out,
                              int32_t *d_status)
{
    if (!ctx) return ALAC_HIP_ParamError;
    alac_hip_format fmt;
    if (int32_t rc = cookie_format(ctx, h_cookie, cookie_size, fmt)) return rc;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!d_out) return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if ((uintptr_t)d_out & 3) return fail(ctx, ALAC_HIP_ParamError, "misaligned buffer");
    if (channel_stride < (uint64_t)num_packets * fmt.frame_size)
        return fail(ctx, ALAC_HIP_ParamError, "channel_stride below num_packets * frame_size");
    if (channel_stride > UINT64_MAX / sizeof(float) / fmt.num_channels)
        return fail(ctx, ALAC_HIP_ParamError, "channel_stride * channels overflows");
    return decode_impl(ctx, h_cookie, cookie_size, d_stream, d_packet_offsets, num_packets, d_workspace, workspace_bytes,
                       (uint8_t *)d_out, d_num_samples_out, d_status, kPcmFloat, nullptr, channel_stride);
}

// ---- verify: alac_hip_decode with the PCM store sites comparing against the caller's PCM ------------------------------
// Workspace: the decoder's own (dec_layout) + the decoded frame counts; no PCM plane on any path — every kernel that writes
// PCM in alac_hip_decode has an instantiation that compares there instead (alac_verify.hpp), the lane decoder's too.
// The decoded frame counts sit in FRONT of the decoder's workspace: the decoder takes everything behind its own layout as
// staging words, so a longer stream only needs a larger workspace here too.
static uint64_t verify_ns_bytes(uint32_t numPackets) { return align_up((uint64_t)numPackets * 4, 256); }

uint64_t alac_hip_verify_workspace_bytes_stream(const alac_hip_format *fmt, uint32_t num_packets, uint64_t stream_bytes)
{
    if (!format_ok(fmt)) return 0;
    return verify_ns_bytes(num_packets) + dec_layout(fmt, num_packets, stream_bytes).total;
}

int32_t alac_hip_verify(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *d_stream,
                        const uint64_t *d_packet_offsets, uint32_t num_packets, const uint8_t *d_pcm_expected,
                        const uint32_t *d_num_samples_expected, void *d_workspace, uint64_t workspace_bytes,
                        uint32_t *d_first_mismatch, int32_t *d_status, uint32_t *d_bad_packets)
{
    if (!ctx) return ALAC_HIP_ParamError;
    alac_hip_format fmt;
    if (int32_t rc = cookie_format(ctx, h_cookie, cookie_size, fmt)) return rc;
    if (!d_bad_packets) return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    if (num_packets == 0) {
        const hipError_t e = hipMemsetAsync(d_bad_packets, 0, 4, ctx->stream);
        return e == hipSuccess ? ALAC_HIP_noErr : fail(ctx, ALAC_HIP_ParamError, "verify launch", e);
    }
    if (!d_stream || !d_packet_offsets || !d_workspace || !d_pcm_expected || !d_first_mismatch || !d_status)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (((uintptr_t)d_workspace & 255) || ((uintptr_t)d_pcm_expected & 3))
        return fail(ctx, ALAC_HIP_ParamError, "misaligned buffer");
    const DecLayout L = dec_layout(&fmt, num_packets);
    const uint64_t nsBytes = verify_ns_bytes(num_packets);
    if (workspace_bytes < nsBytes + L.total) return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    uint8_t *ws = (uint8_t *)d_workspace;
    uint32_t *ns = (uint32_t *)ws;
    hipError_t e = launch_verify_init(d_first_mismatch, num_packets, d_bad_packets, ctx->stream);
    if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "verify launch", e);
    const int32_t rc = decode_impl(ctx, h_cookie, cookie_size, d_stream, d_packet_offsets, num_packets, ws + nsBytes,
                                   workspace_bytes - nsBytes, const_cast<uint8_t *>(d_pcm_expected), ns, d_status,
                                   kPcmVerify, d_first_mismatch);
    if (rc != ALAC_HIP_noErr) return rc;
    e = launch_verify_finish(d_status, ns, d_num_samples_expected, fmt.frame_size, num_packets, d_first_mismatch, d_bad_packets,
                             ctx->stream);
    if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "verify launch", e);
    return ALAC_HIP_noErr;
}

// ---- stage level ---------------------------------------------------------------------------------

int32_t alac_hip_pc_block(alac_hip_ctx *ctx, const int32_t *d_in, int32_t *d_pc, uint32_t num_rows,
                          uint32_t row_stride, int32_t num, int16_t *d_coefs, int32_t numactive, uint32_t chanbits,
                          uint32_t denshift)
{
    if (!ctx || !d_in || !d_pc) return ALAC_HIP_ParamError;
    if (numactive < 0 || numactive > 31 || chanbits < 1 || chanbits > 32 || denshift > 15 || num < 0)
        return fail(ctx, ALAC_HIP_ParamError, "bad pc_block parameters");
    if (numactive != 0 && numactive != 31 && !d_coefs) return fail(ctx, ALAC_HIP_ParamError, "null coefs");
    hipError_t e = launch_pc_block(d_in, d_pc, num_rows, row_stride, num, d_coefs, numactive, chanbits, denshift,
                                   false, ctx->stream, ctx->opt.stageTaps != 0);
    return e == hipSuccess ? ALAC_HIP_noErr : fail(ctx, ALAC_HIP_ParamError, "pc_block launch", e);
}

int32_t alac_hip_unpc_block(alac_hip_ctx *ctx, const int32_t *d_pc, int32_t *d_out, uint32_t num_rows,
                            uint32_t row_stride, int32_t num, int16_t *d_coefs, int32_t numactive,
                            uint32_t chanbits, uint32_t denshift)
{
    if (!ctx || !d_pc || !d_out) return ALAC_HIP_ParamError;
    if (numactive < 0 || numactive > 31 || chanbits < 1 || chanbits > 32 || denshift > 15 || num < 0)
        return fail(ctx, ALAC_HIP_ParamError, "bad unpc_block parameters");
    if (numactive != 0 && numactive != 31 && !d_coefs) return fail(ctx, ALAC_HIP_ParamError, "null coefs");
    hipError_t e = launch_pc_block(d_pc, d_out, num_rows, row_stride, num, d_coefs, numactive, chanbits, denshift,
                                   true, ctx->stream);
    return e == hipSuccess ? ALAC_HIP_noErr : fail(ctx, ALAC_HIP_ParamError, "unpc_block launch", e);
}

int32_t alac_hip_dyn_comp(alac_hip_ctx *ctx, uint32_t mb0, uint32_t pb, uint32_t kb, const int32_t *d_pc,
                          uint32_t num_rows, uint32_t row_stride, int32_t num_samples, int32_t bit_size,
                          uint8_t *d_bits, uint32_t bytes_stride, uint32_t *d_num_bits)
{
    if (!ctx || !d_pc || !d_num_bits) return ALAC_HIP_ParamError;
    if (bit_size < 1 || bit_size > 32 || kb < 1 || kb > 16 || num_samples < 0)  // codec/ag_enc.c:268
        return fail(ctx, ALAC_HIP_ParamError, "bad dyn_comp parameters");
    if (d_bits && ((bytes_stride & 3) || ((uintptr_t)d_bits & 3)))
        return fail(ctx, ALAC_HIP_ParamError, "bit buffer must be 4-byte aligned/strided");
    hipError_t e = launch_dyn_comp(mb0, pb, kb, d_pc, num_rows, row_stride, num_samples, bit_size, d_bits,
                                   bytes_stride, d_num_bits, ctx->stream);
    return e == hipSuccess ? ALAC_HIP_noErr : fail(ctx, ALAC_HIP_ParamError, "dyn_comp launch", e);
}

int32_t alac_hip_dyn_decomp(alac_hip_ctx *ctx, uint32_t mb0, uint32_t pb, uint32_t kb, const uint8_t *d_bits,
                            uint32_t bytes_stride, uint32_t num_rows, int32_t *d_pc, uint32_t row_stride,
                            int32_t num_samples, int32_t max_size, uint32_t *d_num_bits, int32_t *d_status)
{
    if (!ctx || !d_bits || !d_pc || !d_num_bits || !d_status) return ALAC_HIP_ParamError;
    if (max_size < 1 || max_size > 32 || kb < 1 || kb > 16 || num_samples < 0)
        return fail(ctx, ALAC_HIP_ParamError, "bad dyn_decomp parameters");
    hipError_t e = launch_dyn_decomp(mb0, pb, kb, d_bits, bytes_stride, num_rows, d_pc, row_stride, num_samples,
                                     max_size, d_num_bits, d_status, ctx->stream);
    return e == hipSuccess ? ALAC_HIP_noErr : fail(ctx, ALAC_HIP_ParamError, "dyn_decomp launch", e);
}

// ---- host-buffer convenience ---------------------------------------------------------------------

int32_t alac_hip_encode_host_segments(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *h_pcm,
                                      const uint32_t *h_num_samples, uint32_t num_packets, const uint32_t *h_seg_first,
                                      uint32_t num_segments, int16_t *h_state, int32_t state_in, uint8_t *h_out,
                                      uint64_t out_capacity, uint32_t *h_packet_bytes, uint64_t *out_total_bytes)
{
    if (!ctx) return ALAC_HIP_ParamError;
    if (!format_ok(fmt)) return fail(ctx, ALAC_HIP_ParamError, "unsupported format");
    if (out_total_bytes) *out_total_bytes = 0;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!h_pcm || !h_out || !h_packet_bytes || !h_num_samples || !h_seg_first || num_segments == 0)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (int32_t rc = host_segment_refusal(ctx, h_seg_first, num_segments, num_packets)) return rc;

    const uint32_t bpf = fmt->num_channels * bytes_per_sample(fmt->bit_depth);
    const uint32_t np = num_packets, nseg = num_segments;
    const uint64_t pcmBytes = (uint64_t)np * fmt->frame_size * bpf;
    const uint64_t wsBytes = alac_hip_encode_workspace_bytes(fmt, np, ctx->opt.lpc ? np : nseg);
    DevBuf dPcm;
    hipError_t e;
    if ((e = dPcm.alloc(pcmBytes))) return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if ((e = hipMemcpyAsync(dPcm.p, h_pcm, pcmBytes, hipMemcpyHostToDevice, ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    return encode_host_common(ctx, fmt, h_num_samples, np, h_seg_first, nseg, h_state, state_in, h_out, out_capacity,
                              h_packet_bytes, out_total_bytes, wsBytes,
                              [&](uint32_t maxSeg, const uint32_t *ns, const uint32_t *seg, int16_t *state, int32_t stIn,
                                  void *ws, uint8_t *out, uint64_t outMax, uint32_t *sizes, uint64_t *offs) {
                                  return alac_hip_encode_segmented(ctx, fmt, dPcm.p, ns, np, seg, nseg, maxSeg, state, stIn,
                                                                   ws, wsBytes, out, outMax, sizes, offs);
                              });
}

int32_t alac_hip_encode_float_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const float *h_in, uint64_t channel_stride,
                                   uint64_t frame_stride, const uint32_t *h_num_samples, uint32_t num_packets,
                                   const uint32_t *h_seg_first, uint32_t num_segments, int16_t *h_state, int32_t state_in,
                                   uint8_t *h_out, uint64_t out_capacity, uint32_t *h_packet_bytes, uint64_t *out_total_bytes,
                                   uint32_t *h_clipped)
{
    if (!ctx) return ALAC_HIP_ParamError;
    if (!format_ok(fmt)) return fail(ctx, ALAC_HIP_ParamError, "unsupported format");
    if (out_total_bytes) *out_total_bytes = 0;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!h_in || !h_out || !h_packet_bytes || !h_num_samples || !h_seg_first || num_segments == 0)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (int32_t rc = host_segment_refusal(ctx, h_seg_first, num_segments, num_packets)) return rc;
    const uint32_t np = num_packets, nseg = num_segments, fs = fmt->frame_size;
    // the floats the conversion reads lie in [0, span): up to the last frame a packet's num_samples covers.  The same
    // strides then address the copy on the device (alac_hip_encode_float checks them).
    uint64_t span = 0;
    for (uint32_t p = 0; p < np; p++) {
        const uint32_t n = h_num_samples[p] < fs ? h_num_samples[p] : fs;
        if (!n) continue;
        uint64_t rows, cols, last;
        if (__builtin_mul_overflow((uint64_t)(fmt->num_channels - 1), channel_stride, &rows) ||
            __builtin_mul_overflow((uint64_t)p * fs + n - 1, frame_stride, &cols) || __builtin_add_overflow(rows, cols, &last) ||
            last >= UINT64_MAX / sizeof(float))
            return fail(ctx, ALAC_HIP_ParamError, "the largest index into h_in overflows 64 bits");
        span = last + 1 > span ? last + 1 : span;
    }
    const uint64_t wsBytes = alac_hip_encode_float_workspace_bytes(fmt, np, ctx->opt.lpc ? np : nseg);
    DevBuf dIn, dClip;
    hipError_t e;
    if ((e = dIn.alloc(span * sizeof(float))) || (e = dClip.alloc(np * 4ull)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if ((e = hipMemcpyAsync(dIn.p, h_in, span * sizeof(float), hipMemcpyHostToDevice, ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    int32_t rc = encode_host_common(
        ctx, fmt, h_num_samples, np, h_seg_first, nseg, h_state, state_in, h_out, out_capacity, h_packet_bytes,
        out_total_bytes, wsBytes,
        [&](uint32_t maxSeg, const uint32_t *ns, const uint32_t *seg, int16_t *state, int32_t stIn, void *ws, uint8_t *out,
            uint64_t outMax, uint32_t *sizes, uint64_t *offs) {
            return alac_hip_encode_float(ctx, fmt, (const float *)dIn.p, channel_stride, frame_stride, ns, np, seg, nseg, maxSeg,
                                         state, stIn, ws, wsBytes, out, outMax, sizes, offs,
                                         h_clipped ? (uint32_t *)dClip.p : nullptr);
        });
    if (rc != ALAC_HIP_noErr || !h_clipped) return rc;
    if ((e = hipMemcpyAsync(h_clipped, dClip.p, np * 4ull, hipMemcpyDeviceToHost, ctx->stream)) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "D2H copy", e);
    return ALAC_HIP_noErr;
}

int32_t alac_hip_encode_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *h_pcm,
                             uint64_t total_samples, uint32_t segment_packets, int16_t *h_state, int32_t state_in,
                             uint8_t *h_out, uint64_t out_capacity, uint32_t *h_packet_bytes,
                             uint64_t *out_total_bytes)
{
    if (!ctx) return ALAC_HIP_ParamError;
    if (!format_ok(fmt)) return fail(ctx, ALAC_HIP_ParamError, "unsupported format");
    if (out_total_bytes) *out_total_bytes = 0;
    if (total_samples == 0) return ALAC_HIP_noErr;
    if (!h_pcm || !h_out || !h_packet_bytes) return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    const uint32_t bpf = fmt->num_channels * bytes_per_sample(fmt->bit_depth);
    const uint64_t np64 = (total_samples + fmt->frame_size - 1) / fmt->frame_size;
    if (np64 > 0x7fffffffull) return fail(ctx, ALAC_HIP_ParamError, "too many packets");
    const uint32_t np = (uint32_t)np64;
    const uint32_t nseg = segment_packets ? (np + segment_packets - 1) / segment_packets : 1;
    std::vector<uint32_t> ns(np, fmt->frame_size), segFirst(nseg + 1);
    ns[np - 1] = (uint32_t)(total_samples - (uint64_t)(np - 1) * fmt->frame_size);
    for (uint32_t s = 0; s <= nseg; s++) {
        uint64_t f = segment_packets ? (uint64_t)s * segment_packets : (s ? np : 0);
        segFirst[s] = (uint32_t)(f < np ? f : np);
    }
    // the last packet may be partial: hand over whole packets (zero padded)
    const uint64_t inBytes = total_samples * bpf, pcmBytes = (uint64_t)np * fmt->frame_size * bpf;
    const void *src = h_pcm;
    std::vector<uint8_t> padded;
    if (inBytes != pcmBytes) {
        padded.assign(pcmBytes, 0);
        memcpy(padded.data(), h_pcm, inBytes);
        src = padded.data();
    }
    return alac_hip_encode_host_segments(ctx, fmt, src, ns.data(), np, segFirst.data(), nseg, h_state, state_in, h_out,
                                         out_capacity, h_packet_bytes, out_total_bytes);
}

int32_t alac_hip_decode_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size,
                             const uint8_t *h_stream, const uint32_t *h_packet_bytes, uint32_t num_packets,
                             uint8_t *h_pcm_out, uint32_t *h_num_samples_out, int32_t *h_status)
{
    if (!ctx) return ALAC_HIP_ParamError;
    alac_hip_format fmt;
    if (alac_hip_format_from_cookie(h_cookie, cookie_size, &fmt) != ALAC_HIP_noErr || !format_ok(&fmt))
        return fail(ctx, ALAC_HIP_ParamError, "bad magic cookie");
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!h_stream || !h_packet_bytes || !h_pcm_out || !h_num_samples_out || !h_status)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    DevStream d;
    if (int32_t rc = upload_stream(ctx, fmt, h_stream, h_packet_bytes, num_packets, d)) return rc;
    const uint64_t pcmBytes = d.pcmBytes;
    const uint64_t wsBytes = alac_hip_decode_workspace_bytes_stream(&fmt, num_packets, d.total);
    DevBuf dWs, dPcm, dNs, dSt;
    hipError_t e;
    if ((e = dWs.alloc(wsBytes)) || (e = dPcm.alloc(pcmBytes)) || (e = dNs.alloc(num_packets * 4ull)) ||
        (e = dSt.alloc(num_packets * 4ull)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    hipStream_t st = ctx->stream;
    if ((e = hipMemsetAsync(dPcm.p, 0, pcmBytes, st))) return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    int32_t rc = alac_hip_decode(ctx, h_cookie, cookie_size, (const uint8_t *)d.bytes.p, (const uint64_t *)d.offs.p,
                                 num_packets, dWs.p, wsBytes, (uint8_t *)dPcm.p, (uint32_t *)dNs.p,
                                 (int32_t *)dSt.p);
    if (rc != ALAC_HIP_noErr) return rc;
    if ((e = hipMemcpyAsync(h_pcm_out, dPcm.p, pcmBytes, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h_num_samples_out, dNs.p, num_packets * 4ull, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h_status, dSt.p, num_packets * 4ull, hipMemcpyDeviceToHost, st)) ||
        (e = hipStreamSynchronize(st)))
        return fail(ctx, ALAC_HIP_ParamError, "decode execution", e);
    return check_handoff(ctx);
}

int32_t alac_hip_decode_float_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size,
                                   const uint8_t *h_stream, const uint32_t *h_packet_bytes, uint32_t num_packets, float *h_out,
                                   uint64_t channel_stride, uint32_t *h_num_samples_out, int32_t *h_status)
{
    if (!ctx) return ALAC_HIP_ParamError;
    alac_hip_format fmt;
    if (alac_hip_format_from_cookie(h_cookie, cookie_size, &fmt) != ALAC_HIP_noErr || !format_ok(&fmt))
        return fail(ctx, ALAC_HIP_ParamError, "bad magic cookie");
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!h_stream || !h_packet_bytes || !h_out || !h_num_samples_out || !h_status)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    const uint64_t row = (uint64_t)num_packets * fmt.frame_size;  // floats of one channel
    if (channel_stride < row) return fail(ctx, ALAC_HIP_ParamError, "channel_stride below num_packets * frame_size");
    if (channel_stride > UINT64_MAX / sizeof(float) / fmt.num_channels)
        return fail(ctx, ALAC_HIP_ParamError, "channel_stride * channels overflows");
    DevStream d;
    if (int32_t rc = upload_stream(ctx, fmt, h_stream, h_packet_bytes, num_packets, d)) return rc;
    // on the device the rows lie back to back; the copy back puts them channel_stride floats apart and leaves the gap alone
    const uint64_t outBytes = row * fmt.num_channels * sizeof(float);
    const uint64_t wsBytes = alac_hip_decode_workspace_bytes_stream(&fmt, num_packets, d.total);
    DevBuf dWs, dOut, dNs, dSt;
    hipError_t e;
    if ((e = dWs.alloc(wsBytes)) || (e = dOut.alloc(outBytes)) || (e = dNs.alloc(num_packets * 4ull)) ||
        (e = dSt.alloc(num_packets * 4ull)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    hipStream_t st = ctx->stream;
    if ((e = hipMemsetAsync(dOut.p, 0, outBytes, st))) return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    int32_t rc = alac_hip_decode_float(ctx, h_cookie, cookie_size, (const uint8_t *)d.bytes.p, (const uint64_t *)d.offs.p,
                                       num_packets, dWs.p, wsBytes, (float *)dOut.p, row, (uint32_t *)dNs.p, (int32_t *)dSt.p);
    if (rc != ALAC_HIP_noErr) return rc;
    if ((e = hipMemcpy2DAsync(h_out, channel_stride * sizeof(float), dOut.p, row * sizeof(float), row * sizeof(float),
                              fmt.num_channels, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h_num_samples_out, dNs.p, num_packets * 4ull, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h_status, dSt.p, num_packets * 4ull, hipMemcpyDeviceToHost, st)) ||
        (e = hipStreamSynchronize(st)))
        return fail(ctx, ALAC_HIP_ParamError, "decode execution", e);
    return check_handoff(ctx);
}
int32_t alac_hip_verify_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *h_stream,
                             const uint32_t *h_packet_bytes, uint32_t num_packets, const uint8_t *h_pcm_expected,
                             const uint32_t *h_num_samples_expected, uint32_t *h_first_mismatch, int32_t *h_status)
{
    if (!ctx) return ALAC_HIP_ParamError;
    alac_hip_format fmt;
    if (alac_hip_format_from_cookie(h_cookie, cookie_size, &fmt) != ALAC_HIP_noErr || !format_ok(&fmt))
        return fail(ctx, ALAC_HIP_ParamError, "bad magic cookie");
    if (num_packets == 0) return 0;
    if (!h_stream || !h_packet_bytes || !h_pcm_expected) return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (num_packets > 0x7fffffffu) return fail(ctx, ALAC_HIP_ParamError, "more packets than the return value counts");
    DevStream d;
    if (int32_t rc = upload_stream(ctx, fmt, h_stream, h_packet_bytes, num_packets, d)) return rc;
    const uint64_t pcmBytes = d.pcmBytes;
    const uint64_t wsBytes = alac_hip_verify_workspace_bytes_stream(&fmt, num_packets, d.total);
    DevBuf dWs, dPcm, dNs, dFm, dSt, dBad;
    hipError_t e;
    if ((e = dWs.alloc(wsBytes)) || (e = dPcm.alloc(pcmBytes)) || (h_num_samples_expected && (e = dNs.alloc(num_packets * 4ull))) ||
        (e = dFm.alloc(num_packets * 4ull)) || (e = dSt.alloc(num_packets * 4ull)) || (e = dBad.alloc(4)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    hipStream_t st = ctx->stream;
    if ((e = hipMemcpyAsync(dPcm.p, h_pcm_expected, pcmBytes, hipMemcpyHostToDevice, st)) ||
        (h_num_samples_expected &&
         (e = hipMemcpyAsync(dNs.p, h_num_samples_expected, num_packets * 4ull, hipMemcpyHostToDevice, st))))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    int32_t rc = alac_hip_verify(ctx, h_cookie, cookie_size, (const uint8_t *)d.bytes.p, (const uint64_t *)d.offs.p, num_packets,
                                 (const uint8_t *)dPcm.p, (const uint32_t *)dNs.p, dWs.p, wsBytes, (uint32_t *)dFm.p,
                                 (int32_t *)dSt.p, (uint32_t *)dBad.p);
    if (rc != ALAC_HIP_noErr) return rc;
    uint32_t bad = 0;
    if ((e = hipMemcpyAsync(&bad, dBad.p, 4, hipMemcpyDeviceToHost, st)) ||
        (h_first_mismatch && (e = hipMemcpyAsync(h_first_mismatch, dFm.p, num_packets * 4ull, hipMemcpyDeviceToHost, st))) ||
        (h_status && (e = hipMemcpyAsync(h_status, dSt.p, num_packets * 4ull, hipMemcpyDeviceToHost, st))) ||
        (e = hipStreamSynchronize(st)))
        return fail(ctx, ALAC_HIP_ParamError, "verify execution", e);
    rc = check_handoff(ctx);
    return rc != ALAC_HIP_noErr ? rc : (int32_t)bad;
}

}  // extern "C"
