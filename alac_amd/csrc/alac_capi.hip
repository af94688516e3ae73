// alac_capi.hip — the extern "C" boundary of libalac_hip.so (declared in include/alac_hip.h).
// Host-side only: argument checks, workspace carving, kernel launches.  No exceptions cross the
// boundary; every HIP failure becomes one of the reference's int32 status codes.
#include "alac_hip.h"
#include "alac_dev.hpp"
#include "alac_kernels.hpp"
#include "alac_verify.hpp"
#include "alac_encode_v1_types.hpp"
#include "alac_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace alacdev;
using namespace alachost;

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
    // alac_hip_float_probe's segment table, or alac_hip_pcm_crc32's range table, on its way to the device: pinned host memory
    // of the context, so that the caller's table is done with when the call returns wherever it lies; tabDone: the last
    // upload from it has finished
    uint64_t *tabHost = nullptr;
    uint64_t tabCap = 0;  // in entries
    hipEvent_t tabDone = nullptr;
    // code-path switches of this context (alac_hip_set_option); defaults from the ALAC_HIP_* environment at creation
    AlacOptions opt;
};

namespace alacdev {

// key -> the variable of its default, slot and the range alac_hip_set_option accepts (include/alac_hip.h documents exactly
// these)
const AlacOptionKey *alac_option_keys(uint32_t *count)
{
    static const AlacOptionKey table[] = {
        {"thru", "ALAC_HIP_THRU", &AlacOptions::thru, -1, 1},
        {"narrow", "ALAC_HIP_NARROW", &AlacOptions::narrow, -1, 1},
        {"split_coder", "ALAC_HIP_SPLIT_CODER", &AlacOptions::splitCoder, 0, 1},
        {"overlap_pos", "ALAC_HIP_OVERLAP_POS", &AlacOptions::overlapPos, 0, 1},
        {"fused", "ALAC_HIP_FUSED", &AlacOptions::fused, 0, 1},
        {"fold", "ALAC_HIP_FOLD", &AlacOptions::fold, 0, 1},
        {"pub_every", "ALAC_HIP_PUB_EVERY", &AlacOptions::pubEvery, 1, 8, true},
        {"fast_mode", nullptr, &AlacOptions::fastMode, 0, 1},
        {"encoder_lane", "ALAC_HIP_ENCODER", &AlacOptions::laneEncoder, 0, 1},
        {"decoder_lane", "ALAC_HIP_DECODER", &AlacOptions::laneDecoder, 0, 1},
        {"dec_fused", "ALAC_HIP_DEC_FUSED", &AlacOptions::decFused, -1, 1},
        {"dec_pair", "ALAC_HIP_DEC_PAIR", &AlacOptions::decPair, 0, 1},
        {"dec_direct", "ALAC_HIP_DEC_DIRECT", &AlacOptions::decDirect, 0, 2},
        {"stage_taps", "ALAC_HIP_STAGE_TAPS", &AlacOptions::stageTaps, 0, 1},
        {"lpc", nullptr, &AlacOptions::lpc, 0, 1},
        {"debug_lose_handoff", "ALAC_HIP_DEBUG_LOSE_HANDOFF", &AlacOptions::loseHandoff, 0, 1},
        {"debug_waves", nullptr, &AlacOptions::debugWaves, 0, 1},
    };
    if (count) *count = (uint32_t)(sizeof(table) / sizeof(table[0]));
    return table;
}

// The defaults of a new context: a key's variable counts when it is an integer inside the key's range
// (ALAC_HIP_ENCODER=lane / ALAC_HIP_DECODER=lane: 1); anything else leaves the built-in default.
AlacOptions alac_options_from_env()
{
    AlacOptions o;
    uint32_t n = 0;
    const AlacOptionKey *t = alac_option_keys(&n);
    for (uint32_t i = 0; i < n; i++) {
        const char *v = t[i].env ? getenv(t[i].env) : nullptr;
        if (!v || !*v) continue;
        const bool lane = t[i].slot == &AlacOptions::laneEncoder || t[i].slot == &AlacOptions::laneDecoder;
        if (lane && strcmp(v, "lane") == 0) v = "1";
        char *end = nullptr;
        const long x = strtol(v, &end, 10);
        if (*end == '\0' && alac_option_accepts(t[i], x)) o.*(t[i].slot) = (int32_t)x;
    }
    return o;
}

bool alac_option_accepts(const AlacOptionKey &k, long v)
{
    return v >= k.lo && v <= k.hi && (!k.pow2 || (v & (v - 1)) == 0);
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

// fail() in the form the staging steps of alac_host.hpp report through
auto on_fail(alac_hip_ctx *ctx) { return [ctx](int32_t code, const char *what, hipError_t e) { return fail(ctx, code, what, e); }; }

bool format_ok(const alac_hip_format *f)
{
    if (!f) return false;
    if (!(f->bit_depth == 16 || f->bit_depth == 20 || f->bit_depth == 24 || f->bit_depth == 32)) return false;
    if (f->num_channels < 1 || f->num_channels > kMaxChannels) return false;
    if (f->frame_size == 0 || f->frame_size > (1u << 20)) return false;
    return true;
}

inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// The ALACSpecificConfig inside a cookie, and the format it holds; nullptr for a cookie the library cannot read.
// ALACDecoder::Init skips legacy 'frma' and 'alac' atoms (codec/ALACDecoder.cu:123-134).
const uint8_t *read_cookie(const uint8_t *ck, uint32_t size, alac_hip_format *out)
{
    if (!ck || !out) return nullptr;
    for (const char *atom : {"frma", "alac"})
        if (size >= 12 && memcmp(ck + 4, atom, 4) == 0) {
            ck += 12;
            size -= 12;
        }
    if (size < 24 || ck[4] > 0) return nullptr;  // compatibleVersion <= kALACVersion (:153)
    out->frame_size = ((uint32_t)ck[0] << 24) | ((uint32_t)ck[1] << 16) | ((uint32_t)ck[2] << 8) | ck[3];
    out->bit_depth = ck[5];
    out->num_channels = ck[9];
    out->sample_rate = ((uint32_t)ck[20] << 24) | ((uint32_t)ck[21] << 16) | ((uint32_t)ck[22] << 8) | ck[23];
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
    // tap-parallel pipeline: residual planes [sample / 4][stream][4] (alac_plane_index.hpp), decision scratch, working state
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
    // whole cells of four rows (plane_rows: at most three rows more per plane), +16 rows: the coder waves read whole 16-row
    // blocks up to the wave's longest chain
    const uint64_t n8 = plane_rows(f->frame_size / 8 + 1) + 16;
    L.resA = off;
    off = align_up(off + (f->num_channels == 2 ? n8 * 5 * lanes * 4 : 0), 256);
    L.resB = off;
    off = align_up(off + n8 * 2 * lanes * 4, 256);
    // final residuals: columns handed out per packet class (k_class_assign), two regions padded to 64 -> up to 128 spare
    L.colsPad = (uint32_t)lanes + 256;  // the two class regions of the final pass are padded to whole waves
    L.resC = off;
    off = align_up(off + (plane_rows(f->frame_size) + 16) * L.colsPad * 4, 256);
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
// SetFastMode has no first-generation form: a call it applies to (`fast`: a 2-channel stream with "fast_mode" = 1) runs on the
// tap-parallel pipeline whatever "encoder_lane" says, so that the bytes are EncodeStereoFast's under every setting.
bool use_lane_encoder(const alac_hip_ctx *ctx, bool fast = false) { return ctx->opt.laneEncoder != 0 && !fast; }

// > 2 channels: the mono / stereo pipeline once per element over a gathered copy of its channels, then the splice
// (alac_multichannel.hip)
alac_hip_format element_format(const alac_hip_format *f, uint32_t channels)
{
    alac_hip_format e = *f;
    e.num_channels = channels;
    return e;
}

// the bytes of num_packets whole packets of packed interleaved PCM
uint64_t packed_pcm_bytes(const alac_hip_format *fmt, uint32_t num_packets)
{
    return (uint64_t)num_packets * fmt->frame_size * fmt->num_channels * bytes_per_sample(fmt->bit_depth);
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
    (void)hipSetDevice(ctx->device);
    if (ctx->vsReady) {
        (void)hipStreamSynchronize(ctx->vs.side[0]);
        (void)hipStreamDestroy(ctx->vs.side[0]);
        for (uint32_t i = 0; i < kSideEvents; i++) {
            (void)hipEventDestroy(ctx->vs.stagger[i]);
            (void)hipEventDestroy(ctx->vs.join[i]);
        }
        (void)hipEventDestroy(ctx->vs.fork);
    }
    if (ctx->mcReady) {
        (void)hipStreamSynchronize(ctx->mcStream);
        (void)hipStreamDestroy(ctx->mcStream);
        (void)hipEventDestroy(ctx->mcFork);
        (void)hipEventDestroy(ctx->mcJoin);
    }
    if (ctx->ownStream && ctx->stream) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamDestroy(ctx->stream);
    }
    if (ctx->errHost) (void)hipHostFree(ctx->errHost);
    if (ctx->tabDone) (void)hipEventDestroy(ctx->tabDone);
    if (ctx->tabHost) (void)hipHostFree(ctx->tabHost);
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
    if (!alac_option_accepts(*k, value)) return fail(ctx, ALAC_HIP_ParamError, "option value outside its documented range");
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

// ---- the source of an encode call: packed PCM, float32 at strides, or integers in containers at strides --------------------
// The largest index a strided source of `channels` channels and `frames` (>= 1) frames can form, (channels - 1) *
// channel_stride + (frames - 1) * frame_stride; false where it does not fit 64 bits.  Each caller compares `last` with its own
// byte range: float_stride_refusal refuses last > UINT64_MAX / 4 (an index of exactly UINT64_MAX / 4 passes); host_span,
// int_source_struct_refusal and float_probe_refusal refuse last >= UINT64_MAX / container.
static bool largest_index(uint32_t channels, uint64_t channel_stride, uint64_t frames, uint64_t frame_stride, uint64_t &last)
{
    uint64_t rows, cols;
    return !__builtin_mul_overflow((uint64_t)(channels - 1), channel_stride, &rows) &&
           !__builtin_mul_overflow(frames - 1, frame_stride, &cols) && !__builtin_add_overflow(rows, cols, &last);
}

// host forms: the containers a call reads lie in [0, span) of the host buffer — up to the last frame a packet's count covers
// (counts null: frame_size); false where that index overflows 64 bits as a byte offset.  The same strides address the device copy.
static bool host_span(const alac_hip_format *fmt, const uint32_t *h_num_samples, uint32_t np, uint64_t channel_stride,
                      uint64_t frame_stride, uint32_t container, uint64_t &span)
{
    const uint32_t fs = fmt->frame_size;
    span = 0;
    for (uint32_t p = 0; p < np; p++) {
        const uint32_t n = h_num_samples && h_num_samples[p] < fs ? h_num_samples[p] : fs;
        uint64_t last;
        if (!n) continue;
        if (!largest_index(fmt->num_channels, channel_stride, (uint64_t)p * fs + n, frame_stride, last) ||
            last >= UINT64_MAX / container)
            return false;
        span = last + 1 > span ? last + 1 : span;
    }
    return true;
}

// the staged integer PCM of a batch (+ 64: slack behind the last packet, like the gathered copies of a > 2-channel batch)
static uint64_t float_stage_bytes(const alac_hip_format *fmt, uint32_t num_packets)
{
    return align_up(packed_pcm_bytes(fmt, num_packets) + 64, 256);
}

// the strides of a float call: the largest index the conversion can form must fit 64 bits as a byte offset
static int32_t float_stride_refusal(alac_hip_ctx *ctx, const alac_hip_format *fmt, uint32_t num_packets, uint64_t channel_stride,
                                    uint64_t frame_stride)
{
    if (frame_stride == 0) return fail(ctx, ALAC_HIP_ParamError, "frame_stride 0");
    if (channel_stride == 0 && fmt->num_channels > 1)
        return fail(ctx, ALAC_HIP_ParamError, "channel_stride 0 with more than one channel");
    uint64_t last;
    if (!largest_index(fmt->num_channels, channel_stride, (uint64_t)num_packets * fmt->frame_size, frame_stride, last) ||
        last > UINT64_MAX / sizeof(float))
        return fail(ctx, ALAC_HIP_ParamError, "the largest index into d_in overflows 64 bits");
    return ALAC_HIP_noErr;
}

// the dither of a call: what is wrong with the caller's struct (nullptr: nothing), and whether it asks for dither at all
static const char *dither_refusal(const alac_hip_format *fmt, const alac_hip_dither *dither, const uint64_t *packet_origin)
{
    if (!dither) return nullptr;
    if (dither->mode > ALAC_HIP_DITHER_TPDF) return "unknown dither mode";
    if (dither->reserved != 0) return "alac_hip_dither.reserved is not 0";
    if (dither->mode == ALAC_HIP_DITHER_NONE) return nullptr;
    if (fmt->bit_depth == 32) return "no dither at 32 bits: a float32 carries nothing below a 32-bit LSB";
    if ((uintptr_t)packet_origin & 7) return "misaligned packet origin table (8 B)";
    return nullptr;
}
static bool dither_on(const alac_hip_dither *dither) { return dither && dither->mode == ALAC_HIP_DITHER_TPDF; }

// the Philox words of a call's dither (checked; nullptr or mode NONE: none), d_origin the device table or nullptr
static bool dither_args(const alac_hip_dither *dither, const uint64_t *d_origin, FloatDitherArgs &dz)
{
    dz = {};
    if (!dither_on(dither)) return false;
    dz.origin = d_origin;
    philox_round_keys(dither->seed, dz.roundKey);
    return true;
}

// what is wrong with an integer source of `channels` channels and `frames` frames; `in` the device or host pointer.  What
// alac_hip_pcm_requantize and alac_hip_int_probe both refuse, and alac_hip_decode_int in its destination.
static int32_t int_source_struct_refusal(alac_hip_ctx *ctx, const void *in, const alac_hip_int_source *src, uint32_t channels,
                                         uint64_t frames)
{
    if (!in || !src) return fail(ctx, ALAC_HIP_ParamError, "null buffer or alac_hip_int_source");
    const uint32_t cb = src->container_bytes, S = src->bits;
    if (cb < 2 || cb > 4) return fail(ctx, ALAC_HIP_ParamError, "container_bytes is not 2, 3 or 4");
    if ((S != 16 && S != 20 && S != 24 && S != 32) || S > 8 * cb)
        return fail(ctx, ALAC_HIP_ParamError, "bits is not 16, 20, 24 or 32, or above 8 * container_bytes");
    if (src->reserved != 0) return fail(ctx, ALAC_HIP_ParamError, "alac_hip_int_source.reserved is not 0");
    if (src->left_justified > 1) return fail(ctx, ALAC_HIP_ParamError, "left_justified is not 0 or 1");
    if (cb != 3 && ((uintptr_t)in & (cb - 1))) return fail(ctx, ALAC_HIP_ParamError, "buffer not aligned to its container");
    if (src->frame_stride == 0) return fail(ctx, ALAC_HIP_ParamError, "frame_stride 0");
    if (src->channel_stride == 0 && channels > 1)
        return fail(ctx, ALAC_HIP_ParamError, "channel_stride 0 with more than one channel");
    uint64_t last;
    if (frames && (!largest_index(channels, src->channel_stride, frames, src->frame_stride, last) || last >= UINT64_MAX / cb))
        return fail(ctx, ALAC_HIP_ParamError, "the largest index into the buffer overflows 64 bits");
    return ALAC_HIP_noErr;
}

// What an encode or conversion call reads.  Packed: whole packets of packed PCM at `in`, nothing else is used.  Float: float32
// at the strides of `lay` (4-byte containers).  Int: containers as the caller's alac_hip_int_source says (`lay` is its copy;
// noLayout: the caller passed none, which source_refusal reports).  Float and Int may carry a dither with its origin table, and
// clip counters (source_dither).  A host form checks the source with the host pointer in `in`, then swaps in what it staged.
enum class SrcKind { Packed, Float, Int };
struct EncodeSource {
    SrcKind kind = SrcKind::Packed;
    const void *in = nullptr;
    alac_hip_int_source lay = {};  // container bytes, bits, justification; the strides in containers
    bool noLayout = false;
    const alac_hip_dither *dither = nullptr;  // nullable; mode NONE: none
    const uint64_t *origin = nullptr;         // [numPackets] or null: read with dither only
    uint32_t *clipped = nullptr;              // [numPackets] or null
};

static EncodeSource packed_source(const void *pcm) { return {SrcKind::Packed, pcm}; }
static EncodeSource float_source(const float *in, uint64_t channel_stride, uint64_t frame_stride)
{
    return {SrcKind::Float, in, {sizeof(float), 32, 0, 0, channel_stride, frame_stride}};
}
static EncodeSource int_source(const void *in, const alac_hip_int_source *src)
{
    return {SrcKind::Int, in, src ? *src : alac_hip_int_source{}, !src};
}

// the dither, origin table and clip counters of a float or integer source; refuses a bad dither struct
static int32_t source_dither(alac_hip_ctx *ctx, const alac_hip_format *fmt, EncodeSource &s, const alac_hip_dither *dither,
                             const uint64_t *packet_origin, uint32_t *clipped)
{
    if (const char *why = dither_refusal(fmt, dither, packet_origin)) return fail(ctx, ALAC_HIP_ParamError, why);
    s.dither = dither, s.origin = packet_origin, s.clipped = clipped;
    return ALAC_HIP_noErr;
}

// what a call with packets refuses in a source on the device (an integer source: wherever it lies)
static int32_t source_refusal(alac_hip_ctx *ctx, const EncodeSource &s, const alac_hip_format *fmt, uint32_t num_packets)
{
    switch (s.kind) {
    case SrcKind::Packed:
        break;
    case SrcKind::Float:
        if (!s.in) return fail(ctx, ALAC_HIP_ParamError, "null d_in");
        if ((uintptr_t)s.in & 3) return fail(ctx, ALAC_HIP_ParamError, "misaligned d_in (4 B)");
        return float_stride_refusal(ctx, fmt, num_packets, s.lay.channel_stride, s.lay.frame_stride);
    case SrcKind::Int:
        if (int32_t rc = int_source_struct_refusal(ctx, s.in, s.noLayout ? nullptr : &s.lay, fmt->num_channels,
                                                   (uint64_t)num_packets * fmt->frame_size))
            return rc;
        if (dither_on(s.dither) && fmt->bit_depth >= s.lay.bits)
            return fail(ctx, ALAC_HIP_ParamError, "dither where the target depth is not below the source's: nothing is rounded");
    }
    return ALAC_HIP_noErr;
}

// host forms: what a call with packets refuses in a source in host memory (of floats no alignment), and the bytes of it the call
// may read.  Floats: an index that overflows inside the packets' counts is reported for h_in, one only whole packets reach for d_in.
static int32_t source_host_span_bytes(alac_hip_ctx *ctx, const EncodeSource &s, const alac_hip_format *fmt,
                                      const uint32_t *h_num_samples, uint32_t num_packets, uint64_t &bytes)
{
    uint64_t span = 0;
    switch (s.kind) {
    case SrcKind::Packed:
        bytes = packed_pcm_bytes(fmt, num_packets);
        break;
    case SrcKind::Float:
        if (!host_span(fmt, h_num_samples, num_packets, s.lay.channel_stride, s.lay.frame_stride, sizeof(float), span))
            return fail(ctx, ALAC_HIP_ParamError, "the largest index into h_in overflows 64 bits");
        bytes = span * sizeof(float);
        return float_stride_refusal(ctx, fmt, num_packets, s.lay.channel_stride, s.lay.frame_stride);
    case SrcKind::Int:
        if (int32_t rc = source_refusal(ctx, s, fmt, num_packets)) return rc;
        // (no packet reaches further than the whole packets source_refusal has measured)
        if (!host_span(fmt, h_num_samples, num_packets, s.lay.channel_stride, s.lay.frame_stride, s.lay.container_bytes, span))
            return fail(ctx, ALAC_HIP_ParamError, "the largest index into the buffer overflows 64 bits");
        bytes = span * s.lay.container_bytes;
    }
    return ALAC_HIP_noErr;
}

// the conversion of a (checked) float or integer source into packed PCM at `pcm`, enqueued on `st`; a packed source: nothing
static int32_t source_convert(alac_hip_ctx *ctx, const EncodeSource &s, const alac_hip_format &fmt, hipStream_t st,
                              const uint32_t *d_num_samples, uint32_t np, void *pcm)
{
    FloatDitherArgs dz;
    const FloatDitherArgs *dither = s.kind != SrcKind::Packed && dither_args(s.dither, s.origin, dz) ? &dz : nullptr;
    switch (s.kind) {
    case SrcKind::Packed:
        break;
    case SrcKind::Float: {
        const FloatInArgs a{(const float *)s.in, s.lay.channel_stride, s.lay.frame_stride, d_num_samples, np, fmt.frame_size,
                            fmt.num_channels, (uint8_t *)pcm, s.clipped};
        if (hipError_t e = launch_float_to_pcm(fmt.bit_depth, a, st, dither))
            return fail(ctx, ALAC_HIP_ParamError, "float conversion launch", e);
        break;
    }
    case SrcKind::Int: {
        const PcmInArgs a{s.in, s.lay.channel_stride, s.lay.frame_stride, d_num_samples, np, fmt.frame_size, fmt.num_channels,
                          s.lay.container_bytes, s.lay.bits, s.lay.left_justified, (uint8_t *)pcm, s.clipped};
        if (hipError_t e = launch_pcm_requantize(fmt.bit_depth, a, st, dither))
            return fail(ctx, ALAC_HIP_ParamError, "integer conversion launch", e);
    }
    }
    return ALAC_HIP_noErr;
}

// ---- encode: each public call is checked and described once; encode_impl runs the description ----------------------------
// How a call knows its longest segment (the tap-parallel pipeline runs once per packet position of a segment)
enum class SegKind {
    Host,    // no table (1), or a table the library read back and checked on the host: no device check
    Bound,   // the caller's max_segment_packets: the kernels check the table against it (launch_check_segments)
    Unread,  // a table without a bound: the tap-parallel path reads it back (a host wait)
};

// One encode batch.  An entry point fills it by steps: encode_format (the format, the stream, LPC and fast mode of the context,
// and the source: packed_source / float_source / int_source), source_dither, encode_tables, encode_state, encode_buffers;
// encode_pcm then says where the kernels read packed PCM.
struct EncodeCall {
    alac_hip_format fmt;
    EncodeSource src;
    const void *pcm;  // a packed source itself, else the stage the conversion fills
    const uint32_t *numSamples;
    uint32_t numPackets;
    const uint32_t *segFirst;  // nullptr: every packet is its own segment (in LPC mode whatever table the caller passes)
    uint32_t numSegments;      // numPackets without a table
    SegKind segKind;
    uint32_t maxSeg;           // Host: the longest segment; Bound: the caller's bound (clamped to numPackets where used)
    int16_t *state;            // nullptr in LPC mode: the coefficient state is neither read nor written
    int32_t stateIn;
    uint8_t *ws, *out;
    uint32_t *packetBytes;
    uint64_t *offsets;
    hipStream_t stream;
    bool lpc;
    bool fast;   // SetFastMode applies (2-channel streams; not the stereo elements of a 3..8-channel stream)
    bool timed;  // may consume a slot of the armed stage timing
};

// the format, the options and the source: refuses a null context and a format the library does not encode
static int32_t encode_format(alac_hip_ctx *ctx, const alac_hip_format *fmt, const EncodeSource &src, EncodeCall &c)
{
    if (!ctx) return ALAC_HIP_ParamError;
    if (!format_ok(fmt)) return fail(ctx, ALAC_HIP_ParamError, "unsupported format");
    c.fmt = *fmt, c.src = src, c.stream = ctx->stream;
    c.lpc = ctx->opt.lpc != 0, c.fast = ctx->opt.fastMode != 0, c.timed = true;
    return ALAC_HIP_noErr;
}

// the tables (after the options: LPC mode ignores the caller's segment table); max_segment_packets: 0 for none
static void encode_tables(EncodeCall &c, const uint32_t *num_samples, uint32_t num_packets, const uint32_t *seg_first,
                          uint32_t num_segments, uint32_t max_segment_packets)
{
    c.numSamples = num_samples, c.numPackets = num_packets, c.segFirst = c.lpc ? nullptr : seg_first;
    c.numSegments = c.segFirst ? num_segments : num_packets;
    c.segKind = !c.segFirst ? SegKind::Host : max_segment_packets ? SegKind::Bound : SegKind::Unread;
    c.maxSeg = c.segFirst ? max_segment_packets : 1;
}

// the coefficient state (after the options: LPC mode ignores it)
static void encode_state(EncodeCall &c, int16_t *state, int32_t state_in)
{
    c.state = c.lpc ? nullptr : state, c.stateIn = c.lpc ? 0 : state_in;
}

// the workspace and the outputs on the device
static void encode_buffers(EncodeCall &c, void *ws, uint8_t *out, uint32_t *packet_bytes, uint64_t *offsets)
{
    c.ws = (uint8_t *)ws, c.out = out, c.packetBytes = packet_bytes, c.offsets = offsets;
}

// where the kernels read packed PCM: a packed source itself, else the stage behind encBytes bytes of workspace (null with it)
static void encode_pcm(EncodeCall &c, uint64_t encBytes)
{
    c.pcm = c.src.kind == SrcKind::Packed ? c.src.in : c.ws ? c.ws + encBytes : nullptr;
}

// The refusals of an encode call in their order; 0 when it may go ahead (num_packets = 0: after the option refusals).
// num_segments: resolved (num_packets without a table and in LPC mode).  b: the call with the caller's device buffers, which
// are checked too (nulls, alignment, workspace, output capacity); nullptr for the host forms, which allocate them themselves.
static int32_t encode_refusal(alac_hip_ctx *ctx, const alac_hip_format *fmt, uint32_t np, uint32_t num_segments,
                              const EncodeCall *b, uint64_t workspace_bytes, uint64_t out_capacity)
{
    const bool mc = fmt->num_channels > 2, lpc = ctx->opt.lpc != 0;
    if (mc && lpc) return fail(ctx, ALAC_HIP_ParamError, "option lpc: mono and stereo streams only");
    if (lpc) {
        if (ctx->opt.fastMode) return fail(ctx, ALAC_HIP_ParamError, "options lpc and fast_mode exclude each other");
        if ((uint64_t)fmt->frame_size * fmt->num_channels * 4 > 65536)
            return fail(ctx, ALAC_HIP_ParamError, "option lpc: frame_size x channels above 16 384");
    }
    if (np == 0) return ALAC_HIP_noErr;
    if (b && (!b->pcm || !b->ws || !b->out || !b->packetBytes || !b->offsets)) return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (num_segments == 0 || num_segments > np) return fail(ctx, ALAC_HIP_ParamError, "bad segment count");
    if (mc) {
        if (b && ((uintptr_t)b->ws & 255)) return fail(ctx, ALAC_HIP_ParamError, "misaligned workspace (256 B)");
        if ((uint64_t)np * kMaxChannels > 0x7fffffffull) return fail(ctx, ALAC_HIP_ParamError, "too many packets");
        if (b && workspace_bytes < mc_layout(fmt, np, num_segments).total)
            return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    } else if (b) {
        if (((uintptr_t)b->out & 3) || ((uintptr_t)b->ws & 255) || ((uintptr_t)b->pcm & 15))
            return fail(ctx, ALAC_HIP_ParamError, "misaligned buffer (out 4 B, pcm 16 B, workspace 256 B)");
        if (workspace_bytes < enc_layout(fmt, np, num_segments).total + (lpc ? lpc_table_bytes(np) : 0))
            return fail(ctx, ALAC_HIP_ParamError, lpc ? "workspace too small (option lpc: size it for num_segments = num_packets)"
                                                      : "workspace too small");
    }
    if (b && out_capacity < max_output_bytes(fmt, np))
        return fail(ctx, ALAC_HIP_ParamError, "output capacity below alac_hip_encode_max_output_bytes");
    return ALAC_HIP_noErr;
}

// the longest segment of a device segment table, read back (a host wait on `st`); refuses a table that is not ascending
// inside [0, num_packets]
static int32_t read_max_segment(alac_hip_ctx *ctx, hipStream_t st, const uint32_t *d_seg_first, uint32_t num_segments,
                                uint32_t num_packets, uint32_t &maxSeg)
{
    std::vector<uint32_t> sf(num_segments + 1);
    if (hipMemcpyAsync(sf.data(), d_seg_first, (num_segments + 1) * 4ull, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(ctx, ALAC_HIP_ParamError, "reading d_seg_first");
    maxSeg = 0;
    for (uint32_t s = 0; s < num_segments; s++) {
        if (sf[s + 1] < sf[s] || sf[s + 1] > num_packets) return fail(ctx, ALAC_HIP_ParamError, "bad d_seg_first");
        maxSeg = sf[s + 1] - sf[s] > maxSeg ? sf[s + 1] - sf[s] : maxSeg;
    }
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
    // producers publish after every pub_every tiles (1, 2, 4 or 8), rows written through: bit 31, a release fence per publish,
    // stays clear (it cost ~11 us each)
    A.pubMask = (uint32_t)ctx->opt.pubEvery - 1u;
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

// one mono / stereo batch
static int32_t encode_core(alac_hip_ctx *ctx, const EncodeCall &c)
{
    const alac_hip_format *fmt = &c.fmt;
    const uint32_t num_packets = c.numPackets;
    const EncLayout L = enc_layout(fmt, num_packets, c.numSegments);
    uint8_t *ws = c.ws;
    // a table with the caller's bound is not read back (no host wait): the kernels test every entry they use, and a table that
    // contradicts the bound fails the next synchronize
    const bool bound = c.segKind == SegKind::Bound;
    const EncodeArgs ea{(const uint8_t *)c.pcm, c.numSamples, c.segFirst, c.numSegments, fmt->frame_size, c.state, c.stateIn,
                        (int32_t *)(ws + L.pred), L.predStride, (uint32_t *)(ws + L.bitWords), L.wcap, (PacketRec *)(ws + L.recs),
                        c.packetBytes, num_packets, bound ? (c.maxSeg < num_packets ? c.maxSeg : num_packets) : 0xffffffffu,
                        bound ? (uint32_t *)(ws + L.segBad) : nullptr};
    PackArgs pa{ea.pcm, ea.recs, ea.bitWords, L.wcap, fmt->frame_size, c.offsets, c.out, ea.segBad};
    constexpr uint32_t EV = kEventBlocks * (kNumStages + 1);
    hipEvent_t *ev = nullptr;
    if (c.timed && ctx->profile && (uint64_t)(ctx->profCalls + 1) * EV <= ctx->events.size())
        ev = &ctx->events[ctx->profCalls++ * EV];
    const bool lane = use_lane_encoder(ctx, c.fast && fmt->num_channels == 2);
    if (ev) ctx->profLane.push_back(lane);
    hipError_t e;
    // the caller's bound on the segment length is checked on the device whatever kernels run
    if (bound && (e = launch_check_segments(c.segFirst, c.numSegments, num_packets, ea.segMax, ctx->errDev ? ctx->errDev + 1 : nullptr,
                                            ea.segBad, c.stream)))
        return fail(ctx, ALAC_HIP_ParamError, "segment check launch", e);
    if (lane) {
        e = launch_encode(fmt->bit_depth, fmt->num_channels, ea, pa, num_packets, c.stream, ev ? ev + (kNumStages + 1) : nullptr);
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
        uint32_t maxSeg = bound ? ea.segMax : c.maxSeg;
        if (c.segKind == SegKind::Unread)
            if (int32_t rc = read_max_segment(ctx, c.stream, c.segFirst, c.numSegments, num_packets, maxSeg)) return rc;
        AlacOptions opt = ctx->opt;
        opt.fastMode = c.fast ? 1 : 0;
        const V1Plan P = v1_plan(fmt->num_channels, c.numSegments, maxSeg, fmt->frame_size, opt);
        const V1Args A = v1_args(ctx, ea, L, ws, P, c.state == nullptr);
        // rows that hold no caller state and are not taken as constants (V1Args::virgin) get init_coefs first
        const bool initState = !(c.state && c.stateIn) && !A.virgin;
        e = launch_encode_v1(fmt->bit_depth, fmt->num_channels, A, P, initState, pa, ctx->vs, num_packets, maxSeg, c.stream, ev);
    }
    if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "encode launch", e);
    if (c.lpc) {
        // Apple's independent packets are in the records and bit strings: the LPC candidates replace channels they beat,
        // then the sizes are scanned and the packets packed again, with the LPC headers
        const LpcArgs la{ea.pcm, fmt->frame_size, ea.recs, c.packetBytes, ea.bitWords, L.wcap, (LpcChan *)(ws + L.total)};
        e = launch_lpc(fmt->bit_depth, fmt->num_channels, la, num_packets, c.stream);
        if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "lpc launch", e);
        pa.lpc = la.lpc;
        e = launch_scan_pack(fmt->bit_depth, fmt->num_channels, c.packetBytes, pa, num_packets, c.stream, nullptr);
        if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "lpc pack launch", e);
    }
    return ALAC_HIP_noErr;
}

// 3..8 channels: each element group (stereo, mono) as one batch of its own, then the splice
static int32_t encode_elements(alac_hip_ctx *ctx, const EncodeCall &c)
{
    const alac_hip_format *fmt = &c.fmt;
    const uint32_t num_packets = c.numPackets;
    const McLayout M = mc_layout(fmt, num_packets, c.numSegments);
    uint8_t *ws = c.ws;
    const uint32_t bps = bytes_per_sample(fmt->bit_depth);

    // the stereo batch runs on the call's stream, the mono batch beside it on a second stream (both are bound by the latency
    // of one wave, not by the machine)
    const bool side = M.g[0].count && M.g[1].count;
    if (side && !ensure_second_stream(ctx)) return fail(ctx, ALAC_HIP_MemFullError, "creating the second stream");
    hipError_t e;
    if (side && ((e = hipEventRecord(ctx->mcFork, c.stream)) || (e = hipStreamWaitEvent(ctx->mcStream, ctx->mcFork, 0))))
        return fail(ctx, ALAC_HIP_ParamError, "forking the second stream", e);
    int32_t rc = ALAC_HIP_noErr;
    hipError_t copyErr = hipSuccess;
    for (int gi = 0; gi < 2 && rc == ALAC_HIP_noErr; gi++) {
        const McGroup &G = M.g[gi];
        if (!G.count) continue;
        hipStream_t st = (side && gi == 1) ? ctx->mcStream : c.stream;
        const uint64_t elemPcm = (uint64_t)num_packets * fmt->frame_size * G.channels * bps;
        e = hipSuccess;
        for (uint32_t k = 0; k < G.count && e == hipSuccess; k++)
            e = launch_mc_gather((const uint8_t *)c.pcm, ws + G.gather + k * elemPcm, c.numSamples, num_packets, fmt->frame_size,
                                 fmt->num_channels, M.el[G.elem[k]].first, G.channels, bps, st);
        uint32_t *ns = c.numSamples ? (uint32_t *)(ws + G.ns) : nullptr;
        uint32_t *seg = c.segFirst ? (uint32_t *)(ws + G.seg) : nullptr;
        if (e == hipSuccess) e = launch_mc_tables(c.numSamples, num_packets, c.segFirst, c.numSegments, G.count, ns, seg, st);
        if (e != hipSuccess) {
            rc = fail(ctx, ALAC_HIP_ParamError, "element gather launch", e);
            break;
        }
        // coefficient rows: the caller's [element][segment][64] <-> the batch's [k][segment][64]
        int16_t *gstate = c.state ? (int16_t *)(ws + G.state) : nullptr;
        const uint64_t rowBytes = (uint64_t)c.numSegments * ALAC_HIP_STATE_INT16 * 2;
        if (gstate && c.stateIn)
            for (uint32_t k = 0; k < G.count && copyErr == hipSuccess; k++)
                copyErr = hipMemcpyAsync((uint8_t *)gstate + k * rowBytes, (const uint8_t *)c.state + G.elem[k] * rowBytes,
                                         rowBytes, hipMemcpyDeviceToDevice, st);
        // the group's segment tables are built on the device and keep the call's bound: with none they are read back
        // (SegKind::Unread).  SetFastMode is consulted for 2-channel STREAMS only (codec/ALACEncoder.cu:998-1001): the stereo
        // elements of a > 2-channel stream are searched like everything else; no LPC (refused), no stage timing.
        EncodeCall g;
        g.fmt = element_format(fmt, G.channels), g.src = packed_source(ws + G.gather), g.stream = st;
        g.lpc = g.fast = g.timed = false;
        encode_tables(g, ns, G.count * num_packets, seg, G.count * c.numSegments, c.maxSeg);
        encode_state(g, gstate, c.stateIn);
        encode_buffers(g, ws + G.sub, ws + G.out, (uint32_t *)(ws + G.sizes), (uint64_t *)(ws + G.offs));
        encode_pcm(g, 0);
        rc = encode_core(ctx, g);
        if (gstate && rc == ALAC_HIP_noErr)
            for (uint32_t k = 0; k < G.count && copyErr == hipSuccess; k++)
                copyErr = hipMemcpyAsync((uint8_t *)c.state + G.elem[k] * rowBytes, (const uint8_t *)gstate + k * rowBytes,
                                         rowBytes, hipMemcpyDeviceToDevice, st);
    }
    // the second stream is joined whatever happened, so the call's stream stays the only one to wait on
    if (side && ((e = hipEventRecord(ctx->mcJoin, ctx->mcStream)) || (e = hipStreamWaitEvent(c.stream, ctx->mcJoin, 0))) &&
        rc == ALAC_HIP_noErr)
        rc = fail(ctx, ALAC_HIP_ParamError, "joining the second stream", e);
    if (rc != ALAC_HIP_noErr) return rc;
    if (copyErr != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "coefficient state copy", copyErr);
    McSpliceArgs sa;
    sa.numElements = M.numElements;
    sa.numPackets = num_packets;
    for (uint32_t el = 0; el < M.numElements; el++) {
        const McGroup &G = M.g[M.groupOf[el]];
        sa.el[el] = M.el[el];
        sa.src[el] = ws + G.out;
        sa.srcOffsets[el] = (const uint64_t *)(ws + G.offs) + (uint64_t)M.indexInGroup[el] * num_packets;
    }
    sa.elemBits = (uint32_t *)(ws + M.elemBits);
    sa.packetBytes = c.packetBytes;
    sa.offsets = c.offsets;
    sa.out = c.out;
    e = launch_mc_splice(sa, c.stream);
    if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "splice launch", e);
    return ALAC_HIP_noErr;
}

// a (checked) call's work on its stream: the conversion of its source into the stage, if it has one, then the encode
static int32_t encode_run(alac_hip_ctx *ctx, const EncodeCall &c)
{
    if (int32_t rc = source_convert(ctx, c.src, c.fmt, c.stream, c.numSamples, c.numPackets, (void *)c.pcm)) return rc;
    return (c.fmt.num_channels > 2 ? encode_elements : encode_core)(ctx, c);
}

// Every device form behind its description.  With no packets only the option refusals count.  A float or integer source is
// checked in front of the buffers; its stage is the last whole 256-byte blocks of the workspace, the encoder gets the rest.
static int32_t encode_impl(alac_hip_ctx *ctx, EncodeCall &c, uint64_t workspace_bytes, uint64_t out_capacity)
{
    const alac_hip_format *fmt = &c.fmt;
    const uint32_t num_packets = c.numPackets;
    const bool staged = c.src.kind != SrcKind::Packed;
    if (num_packets == 0) return encode_refusal(ctx, fmt, 0, c.numSegments, &c, workspace_bytes, out_capacity);
    uint64_t encBytes = workspace_bytes;
    if (staged) {
        if (int32_t rc = source_refusal(ctx, c.src, fmt, num_packets)) return rc;
        const uint64_t stage = float_stage_bytes(fmt, num_packets);
        if (workspace_bytes < stage) return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
        encBytes = (workspace_bytes - stage) & ~255ull;
    }
    encode_pcm(c, encBytes);
    if (int32_t rc = encode_refusal(ctx, fmt, num_packets, c.numSegments, &c, encBytes, out_capacity)) return rc;
    // tap-parallel path behind a conversion: a table without a bound is read back before anything is enqueued, and handed on
    if (staged && c.segKind == SegKind::Unread && fmt->num_channels <= 2 &&
        !use_lane_encoder(ctx, c.fast && fmt->num_channels == 2)) {
        if (int32_t rc = read_max_segment(ctx, c.stream, c.segFirst, c.numSegments, num_packets, c.maxSeg)) return rc;
        c.segKind = SegKind::Host;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    return encode_run(ctx, c);
}

int32_t alac_hip_encode_segmented(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_pcm,
                                  const uint32_t *d_num_samples, uint32_t num_packets, const uint32_t *d_seg_first,
                                  uint32_t num_segments, uint32_t max_segment_packets, int16_t *d_state, int32_t state_in,
                                  void *d_workspace, uint64_t workspace_bytes, uint8_t *d_out, uint64_t out_capacity,
                                  uint32_t *d_packet_bytes, uint64_t *d_packet_offsets)
{
    EncodeCall c;
    if (int32_t rc = encode_format(ctx, fmt, packed_source(d_pcm), c)) return rc;
    encode_tables(c, d_num_samples, num_packets, d_seg_first, num_segments, max_segment_packets);
    encode_state(c, d_state, state_in);
    encode_buffers(c, d_workspace, d_out, d_packet_bytes, d_packet_offsets);
    return encode_impl(ctx, c, workspace_bytes, out_capacity);
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

// ---- float32 input: quantize into a stage at the end of the workspace, then encode from it ---------------------------------
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
    return alac_hip_encode_float_dither(ctx, fmt, d_in, channel_stride, frame_stride, d_num_samples, num_packets, d_seg_first,
                                        num_segments, max_segment_packets, d_state, state_in, d_workspace, workspace_bytes,
                                        d_out, out_capacity, d_packet_bytes, d_packet_offsets, d_clipped, nullptr, nullptr);
}

int32_t alac_hip_encode_float_dither(alac_hip_ctx *ctx, const alac_hip_format *fmt, const float *d_in, uint64_t channel_stride,
                                     uint64_t frame_stride, const uint32_t *d_num_samples, uint32_t num_packets,
                                     const uint32_t *d_seg_first, uint32_t num_segments, uint32_t max_segment_packets,
                                     int16_t *d_state, int32_t state_in, void *d_workspace, uint64_t workspace_bytes,
                                     uint8_t *d_out, uint64_t out_capacity, uint32_t *d_packet_bytes,
                                     uint64_t *d_packet_offsets, uint32_t *d_clipped, const alac_hip_dither *dither,
                                     const uint64_t *d_packet_origin)
{
    EncodeCall c;
    if (int32_t rc = encode_format(ctx, fmt, float_source(d_in, channel_stride, frame_stride), c)) return rc;
    if (int32_t rc = source_dither(ctx, fmt, c.src, dither, d_packet_origin, d_clipped)) return rc;
    encode_tables(c, d_num_samples, num_packets, d_seg_first, num_segments, max_segment_packets);
    encode_state(c, d_state, state_in);
    encode_buffers(c, d_workspace, d_out, d_packet_bytes, d_packet_offsets);
    return encode_impl(ctx, c, workspace_bytes, out_capacity);
}

// ---- integer input of any layout, container and depth: requantize by the integer rule, then encode from the result ------
int32_t alac_hip_pcm_requantize(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_in, const alac_hip_int_source *src,
                                const uint32_t *d_num_samples, uint32_t num_packets, uint8_t *d_pcm_out, uint64_t pcm_capacity,
                                uint32_t *d_clipped, const alac_hip_dither *dither, const uint64_t *d_packet_origin)
{
    if (!ctx) return ALAC_HIP_ParamError;
    if (!format_ok(fmt)) return fail(ctx, ALAC_HIP_ParamError, "unsupported format");
    EncodeSource s = int_source(d_in, src);
    if (int32_t rc = source_dither(ctx, fmt, s, dither, d_packet_origin, d_clipped)) return rc;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (int32_t rc = source_refusal(ctx, s, fmt, num_packets)) return rc;
    if (!d_pcm_out || ((uintptr_t)d_pcm_out & 15)) return fail(ctx, ALAC_HIP_ParamError, "null or misaligned d_pcm_out (16 B)");
    if (pcm_capacity < packed_pcm_bytes(fmt, num_packets))
        return fail(ctx, ALAC_HIP_ParamError, "pcm_capacity below num_packets packets");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    return source_convert(ctx, s, *fmt, ctx->stream, d_num_samples, num_packets, d_pcm_out);
}

uint64_t alac_hip_encode_int_workspace_bytes(const alac_hip_format *fmt, uint32_t num_packets, uint32_t num_segments)
{
    return alac_hip_encode_float_workspace_bytes(fmt, num_packets, num_segments);  // the same stage behind the same workspace
}

int32_t alac_hip_encode_int(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_in, const alac_hip_int_source *src,
                            const uint32_t *d_num_samples, uint32_t num_packets, const uint32_t *d_seg_first,
                            uint32_t num_segments, uint32_t max_segment_packets, int16_t *d_state, int32_t state_in,
                            void *d_workspace, uint64_t workspace_bytes, uint8_t *d_out, uint64_t out_capacity,
                            uint32_t *d_packet_bytes, uint64_t *d_packet_offsets, uint32_t *d_clipped,
                            const alac_hip_dither *dither, const uint64_t *d_packet_origin)
{
    EncodeCall c;
    if (int32_t rc = encode_format(ctx, fmt, int_source(d_in, src), c)) return rc;
    if (int32_t rc = source_dither(ctx, fmt, c.src, dither, d_packet_origin, d_clipped)) return rc;
    encode_tables(c, d_num_samples, num_packets, d_seg_first, num_segments, max_segment_packets);
    encode_state(c, d_state, state_in);
    encode_buffers(c, d_workspace, d_out, d_packet_bytes, d_packet_offsets);
    return encode_impl(ctx, c, workspace_bytes, out_capacity);
}

// ---- float32 probe: the lossless bit depth of float PCM, per segment of frames ---------------------------------------------
uint64_t alac_hip_float_probe_workspace_bytes(uint32_t num_segments)
{
    return num_segments ? align_up(((uint64_t)num_segments + 1) * 8, 256) : 0;
}

// what a probe call refuses in its host segment table; [lo, hi): the frames the segments cover
static int32_t probe_table_refusal(alac_hip_ctx *ctx, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                   uint32_t num_segments, uint64_t &lo, uint64_t &hi)
{
    if (num_segments == 0) return fail(ctx, ALAC_HIP_ParamError, "num_segments 0");
    lo = 0, hi = total_frames;
    if (!h_seg_first_frame)
        return num_segments == 1 ? ALAC_HIP_noErr : fail(ctx, ALAC_HIP_ParamError, "no segment table for more than one segment");
    for (uint32_t s = 0; s < num_segments; s++)
        if (h_seg_first_frame[s] > h_seg_first_frame[s + 1]) return fail(ctx, ALAC_HIP_ParamError, "segment table not ascending");
    if (h_seg_first_frame[num_segments] > total_frames)
        return fail(ctx, ALAC_HIP_ParamError, "segment table ends behind total_frames");
    lo = h_seg_first_frame[0], hi = h_seg_first_frame[num_segments];
    return ALAC_HIP_noErr;
}

// everything alac_hip_float_probe refuses that does not depend on where the buffers live; [lo, hi): the frames the segments
// cover.  Device and host form.
static int32_t float_probe_refusal(alac_hip_ctx *ctx, const float *in, uint32_t num_channels, uint64_t channel_stride,
                                   uint64_t frame_stride, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                   uint32_t num_segments, uint64_t &lo, uint64_t &hi)
{
    if (!in) return fail(ctx, ALAC_HIP_ParamError, "null input");
    if ((uintptr_t)in & 3) return fail(ctx, ALAC_HIP_ParamError, "misaligned input (4 B)");
    if (num_channels < 1 || num_channels > kMaxChannels) return fail(ctx, ALAC_HIP_ParamError, "num_channels outside 1..8");
    if (frame_stride == 0) return fail(ctx, ALAC_HIP_ParamError, "frame_stride 0");
    if (channel_stride == 0 && num_channels > 1)
        return fail(ctx, ALAC_HIP_ParamError, "channel_stride 0 with more than one channel");
    uint64_t last;
    if (total_frames &&
        (!largest_index(num_channels, channel_stride, total_frames, frame_stride, last) || last >= UINT64_MAX / sizeof(float)))
        return fail(ctx, ALAC_HIP_ParamError, "the largest index into the input overflows 64 bits");
    return probe_table_refusal(ctx, total_frames, h_seg_first_frame, num_segments, lo, hi);
}

// The segment table goes to the device through the context's pinned buffer: copied out of the caller's memory here, on the
// host, so the caller may reuse the table at once even where it is pinned memory, from which hipMemcpyAsync reads later.
// A call that follows while the last upload is still in flight waits for that upload (not for the probe behind it).
static hipError_t upload_segment_table(alac_hip_ctx *ctx, const uint64_t *h_table, uint64_t entries, void *d_dst)
{
    hipError_t e;
    if (!ctx->tabDone && (e = hipEventCreateWithFlags(&ctx->tabDone, hipEventDisableTiming))) return e;
    if (ctx->tabHost && (e = hipEventSynchronize(ctx->tabDone))) return e;
    if (entries > ctx->tabCap) {
        if (ctx->tabHost) (void)hipHostFree(ctx->tabHost);
        ctx->tabHost = nullptr, ctx->tabCap = 0;
        const uint64_t cap = entries < 1024 ? 1024 : entries;
        if ((e = hipHostMalloc((void **)&ctx->tabHost, cap * 8, hipHostMallocDefault))) return e;
        ctx->tabCap = cap;
    }
    memcpy(ctx->tabHost, h_table, entries * 8);
    if ((e = hipMemcpyAsync(d_dst, ctx->tabHost, entries * 8, hipMemcpyHostToDevice, ctx->stream))) return e;
    return hipEventRecord(ctx->tabDone, ctx->stream);
}

// what a probe call refuses in its workspace and report pointer; then the device is selected and the table, if there is one,
// is on its way into the workspace
static int32_t probe_table_to_device(alac_hip_ctx *ctx, const uint64_t *h_seg_first_frame, uint32_t num_segments,
                                     void *d_workspace, uint64_t workspace_bytes, const void *d_reports)
{
    if (!d_reports || ((uintptr_t)d_reports & 7)) return fail(ctx, ALAC_HIP_ParamError, "null or misaligned d_reports (8 B)");
    if (workspace_bytes < alac_hip_float_probe_workspace_bytes(num_segments))
        return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    if (h_seg_first_frame && (!d_workspace || ((uintptr_t)d_workspace & 7)))
        return fail(ctx, ALAC_HIP_ParamError, "null or misaligned workspace (8 B)");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    hipError_t e;
    if (h_seg_first_frame && (e = upload_segment_table(ctx, h_seg_first_frame, (uint64_t)num_segments + 1, d_workspace)))
        return fail(ctx, ALAC_HIP_ParamError, "segment table upload", e);
    return ALAC_HIP_noErr;
}

int32_t alac_hip_float_probe(alac_hip_ctx *ctx, const float *d_in, uint32_t num_channels, uint64_t channel_stride,
                             uint64_t frame_stride, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                             uint32_t num_segments, void *d_workspace, uint64_t workspace_bytes,
                             alac_hip_float_report *d_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = float_probe_refusal(ctx, d_in, num_channels, channel_stride, frame_stride, total_frames, h_seg_first_frame,
                                         num_segments, lo, hi))
        return rc;
    if (int32_t rc = probe_table_to_device(ctx, h_seg_first_frame, num_segments, d_workspace, workspace_bytes, d_reports)) return rc;
    hipError_t e;
    const FloatProbeArgs a{d_in, channel_stride, frame_stride, lo, hi, h_seg_first_frame ? (const uint64_t *)d_workspace : nullptr,
                           num_segments, num_channels, (uint32_t *)d_reports};
    if ((e = launch_float_probe(a, ctx->stream))) return fail(ctx, ALAC_HIP_ParamError, "float probe launch", e);
    return ALAC_HIP_noErr;
}

uint32_t alac_hip_float_report_depth(const alac_hip_float_report *r)
{
    if (!r || r->nan || r->over_range || r->need_bits > 32) return 0;
    return r->need_bits <= 16 ? 16 : r->need_bits <= 20 ? 20 : r->need_bits <= 24 ? 24 : 32;
}

// ---- integer probe: the lossless bit depth of integer PCM, per segment of frames ------------------------------------------
uint64_t alac_hip_int_probe_workspace_bytes(uint32_t num_segments)
{
    return alac_hip_float_probe_workspace_bytes(num_segments);  // the same table
}

// everything alac_hip_int_probe refuses that does not depend on where the buffers live.  Device and host form.
static int32_t int_probe_refusal(alac_hip_ctx *ctx, const void *in, const alac_hip_int_source *src, uint32_t num_channels,
                                 uint64_t total_frames, const uint64_t *h_seg_first_frame, uint32_t num_segments, uint64_t &lo,
                                 uint64_t &hi)
{
    if (num_channels < 1 || num_channels > kMaxChannels) return fail(ctx, ALAC_HIP_ParamError, "num_channels outside 1..8");
    if (int32_t rc = int_source_struct_refusal(ctx, in, src, num_channels, total_frames)) return rc;
    return probe_table_refusal(ctx, total_frames, h_seg_first_frame, num_segments, lo, hi);
}

int32_t alac_hip_int_probe(alac_hip_ctx *ctx, const void *d_in, const alac_hip_int_source *src, uint32_t num_channels,
                           uint64_t total_frames, const uint64_t *h_seg_first_frame, uint32_t num_segments, void *d_workspace,
                           uint64_t workspace_bytes, alac_hip_int_report *d_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = int_probe_refusal(ctx, d_in, src, num_channels, total_frames, h_seg_first_frame, num_segments, lo, hi))
        return rc;
    if (int32_t rc = probe_table_to_device(ctx, h_seg_first_frame, num_segments, d_workspace, workspace_bytes, d_reports)) return rc;
    const IntProbeArgs a{d_in, src->channel_stride, src->frame_stride, lo, hi,
                         h_seg_first_frame ? (const uint64_t *)d_workspace : nullptr, num_segments, num_channels,
                         src->container_bytes, src->bits, src->left_justified, (uint32_t *)d_reports};
    if (hipError_t e = launch_int_probe(a, ctx->stream)) return fail(ctx, ALAC_HIP_ParamError, "integer probe launch", e);
    return ALAC_HIP_noErr;
}

uint32_t alac_hip_int_report_depth(const alac_hip_int_report *r)
{
    if (!r || r->out_of_range || r->pad_bits) return 0;
    return r->need_bits <= 16 ? 16 : r->need_bits <= 20 ? 20 : r->need_bits <= 24 ? 24 : 32;
}

// ---- CRC-32 of PCM: the fingerprint of a decode, per range of bytes ---------------------------------------------------------
uint64_t alac_hip_pcm_crc32_workspace_bytes(uint32_t num_ranges)
{
    return num_ranges ? align_up((uint64_t)num_ranges * 16, 256) : 0;
}

// everything alac_hip_pcm_crc32 refuses that does not depend on where the buffers live; [lo, hi): from the first range's
// first byte to the last one's end.  Device and host form.
static int32_t pcm_crc_refusal(alac_hip_ctx *ctx, const void *pcm, uint64_t total_bytes, const uint64_t *h_ranges,
                               uint32_t num_ranges, uint64_t &lo, uint64_t &hi)
{
    if (!pcm && total_bytes) return fail(ctx, ALAC_HIP_ParamError, "null PCM");
    if (num_ranges == 0) return fail(ctx, ALAC_HIP_ParamError, "num_ranges 0");
    lo = 0, hi = total_bytes;
    if (!h_ranges) return num_ranges == 1 ? ALAC_HIP_noErr : fail(ctx, ALAC_HIP_ParamError, "no range table for more than one range");
    uint64_t at = 0;
    for (uint32_t s = 0; s < num_ranges; s++) {
        uint64_t end;
        if (h_ranges[2 * s] < at) return fail(ctx, ALAC_HIP_ParamError, "range table not ascending, or ranges overlap");
        if (__builtin_add_overflow(h_ranges[2 * s], h_ranges[2 * s + 1], &end))
            return fail(ctx, ALAC_HIP_ParamError, "a range's end overflows 64 bits");
        at = end;
    }
    if (at > total_bytes) return fail(ctx, ALAC_HIP_ParamError, "range table ends behind total_bytes");
    lo = h_ranges[0], hi = at;
    return ALAC_HIP_noErr;
}

int32_t alac_hip_pcm_crc32(alac_hip_ctx *ctx, const void *d_pcm, uint64_t total_bytes, const uint64_t *h_ranges,
                           uint32_t num_ranges, void *d_workspace, uint64_t workspace_bytes, alac_hip_pcm_digest *d_digests)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = pcm_crc_refusal(ctx, d_pcm, total_bytes, h_ranges, num_ranges, lo, hi)) return rc;
    if (!d_digests || ((uintptr_t)d_digests & 7)) return fail(ctx, ALAC_HIP_ParamError, "null or misaligned d_digests (8 B)");
    if (h_ranges && workspace_bytes < alac_hip_pcm_crc32_workspace_bytes(num_ranges))
        return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    if (h_ranges && (!d_workspace || ((uintptr_t)d_workspace & 7)))
        return fail(ctx, ALAC_HIP_ParamError, "null or misaligned workspace (8 B)");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    hipError_t e;
    if (h_ranges && (e = upload_segment_table(ctx, h_ranges, (uint64_t)num_ranges * 2, d_workspace)))
        return fail(ctx, ALAC_HIP_ParamError, "range table upload", e);
    const PcmCrcArgs a{(const uint8_t *)d_pcm, lo, hi, h_ranges ? (const uint64_t *)d_workspace : nullptr, num_ranges,
                       (uint32_t *)d_digests};
    if ((e = launch_pcm_crc(a, ctx->stream))) return fail(ctx, ALAC_HIP_ParamError, "pcm crc launch", e);
    return ALAC_HIP_noErr;
}

uint32_t alac_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
    return crc_mul_host(crc_a, crc_x8_pow(len_b)) ^ crc_b;
}

// ---- loudness: BS.1770 energies per 100 ms and the sample peak, per segment of frames ------------------------------------
// the chunks and groups a call can have at most: every segment ends with at most one short chunk and one short group
static void loudness_bounds(uint32_t L, uint64_t total_frames, uint32_t num_segments, uint64_t &chunks, uint64_t &groups)
{
    chunks = total_frames / L + num_segments;
    groups = chunks / kLoudGroup + num_segments;
}

// the workspace: the four tables, the chunks' states, the groups' states, the chunks' sums
struct LoudnessLayout {
    uint64_t tables, state, gstate, partial, total;
};
static LoudnessLayout loudness_layout(uint32_t L, uint32_t num_channels, uint64_t total_frames, uint32_t num_segments)
{
    uint64_t chunks, groups;
    loudness_bounds(L, total_frames, num_segments, chunks, groups);
    LoudnessLayout w;
    w.tables = 0;
    w.state = align_up(4 * ((uint64_t)num_segments + 1) * 8, 256);
    w.gstate = w.state + align_up(chunks * num_channels * 32, 256);
    w.partial = w.gstate + align_up(groups * num_channels * 32, 256);
    w.total = w.partial + align_up(chunks * num_channels * 8, 256) + 256;  // + 256: the arrays start at the next multiple of 32
    return w;
}

uint64_t alac_hip_loudness_workspace_bytes(uint32_t sample_rate, uint32_t num_channels, uint64_t total_frames,
                                           uint32_t num_segments)
{
    if (!loud_rate_ok(sample_rate) || num_channels < 1 || num_channels > kMaxChannels || num_segments == 0) return 0;
    return loudness_layout(loud_chunk_frames(sample_rate), num_channels, total_frames, num_segments).total;
}

// What both loudness calls do behind the source's own refusals (the caller's: int_probe_refusal or float_probe_refusal, which
// leave [lo, hi)): the remaining refusals, then the tables to the device and the passes.  containerBytes 0: float32.
static int32_t loudness_impl(alac_hip_ctx *ctx, LoudArgs a, uint32_t sample_rate, uint64_t total_frames,
                             const uint64_t *h_seg_first_frame, uint64_t lo, uint64_t hi, void *d_workspace,
                             uint64_t workspace_bytes, double *d_energy, uint64_t energy_rows, void *d_reports)
{
    if (!loud_rate_ok(sample_rate)) return fail(ctx, ALAC_HIP_ParamError, "sample rate is not a multiple of 10 in [8000, 384000]");
    if (!d_reports || ((uintptr_t)d_reports & 7)) return fail(ctx, ALAC_HIP_ParamError, "null or misaligned d_reports (8 B)");
    if (!d_energy || ((uintptr_t)d_energy & 7)) return fail(ctx, ALAC_HIP_ParamError, "null or misaligned d_energy (8 B)");
    if (!d_workspace || ((uintptr_t)d_workspace & 7)) return fail(ctx, ALAC_HIP_ParamError, "null or misaligned workspace (8 B)");
    const uint32_t nseg = a.numSegments, L = loud_chunk_frames(sample_rate);
    const uint64_t hop = sample_rate / 10;
    const LoudnessLayout w = loudness_layout(L, a.channels, total_frames, nseg);
    if (workspace_bytes < w.total) return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    // segFirst, rowBase, chunkBase, groupBase, [nseg + 1] each
    std::vector<uint64_t> table(4 * ((size_t)nseg + 1));
    uint64_t *first = table.data(), *row = first + nseg + 1, *chunk = row + nseg + 1, *group = chunk + nseg + 1;
    row[0] = chunk[0] = group[0] = 0;
    for (uint32_t s = 0; s <= nseg; s++) first[s] = h_seg_first_frame ? h_seg_first_frame[s] : (s ? hi : lo);
    for (uint32_t s = 0; s < nseg; s++) {
        const uint64_t n = first[s + 1] - first[s], chunks = (n + L - 1) / L;
        row[s + 1] = row[s] + n / hop;
        chunk[s + 1] = chunk[s] + chunks;
        group[s + 1] = group[s] + (chunks + kLoudGroup - 1) / kLoudGroup;
    }
    if (row[nseg] > 0xffffffffull) return fail(ctx, ALAC_HIP_ParamError, "more than 2^32 - 1 rows");
    if (energy_rows < row[nseg]) return fail(ctx, ALAC_HIP_ParamError, "energy_rows below the table's row count");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    hipError_t e;
    if ((e = upload_segment_table(ctx, table.data(), table.size(), d_workspace)))
        return fail(ctx, ALAC_HIP_ParamError, "segment table upload", e);
    // the tables lie at the workspace's start; the arrays behind them count from the next multiple of 32 bytes
    uint8_t *ws = (uint8_t *)align_up((uint64_t)(uintptr_t)d_workspace, 32);
    a.segFirst = (const uint64_t *)d_workspace;
    a.rowBase = a.segFirst + nseg + 1, a.chunkBase = a.rowBase + nseg + 1, a.groupBase = a.chunkBase + nseg + 1;
    a.L = L, a.chunksPerHop = (uint32_t)(hop / L);
    a.totalRows = row[nseg], a.totalChunks = chunk[nseg], a.totalGroups = group[nseg];
    loud_filter_coefs(sample_rate, a.coef);
    loud_state_maps(a.coef, L, a.M, a.MG);
    a.state = (double *)(ws + w.state), a.gstate = (double *)(ws + w.gstate), a.partial = (double *)(ws + w.partial);
    a.energy = d_energy;
    a.reports = (uint32_t *)d_reports;
    if ((e = launch_loudness(a, ctx->stream))) return fail(ctx, ALAC_HIP_ParamError, "loudness launch", e);
    return ALAC_HIP_noErr;
}

static LoudArgs loudness_source(const void *in, uint64_t channel_stride, uint64_t frame_stride, uint32_t num_segments,
                                uint32_t num_channels, uint32_t container_bytes, uint32_t bits, uint32_t left_justified)
{
    LoudArgs a = {};
    a.in = in, a.channelStride = channel_stride, a.frameStride = frame_stride;
    a.numSegments = num_segments, a.channels = num_channels;
    a.containerBytes = container_bytes, a.srcBits = bits, a.leftJustified = left_justified;
    return a;
}

int32_t alac_hip_loudness_int(alac_hip_ctx *ctx, const void *d_in, const alac_hip_int_source *src, uint32_t num_channels,
                              uint32_t sample_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                              uint32_t num_segments, void *d_workspace, uint64_t workspace_bytes, double *d_energy,
                              uint64_t energy_rows, alac_hip_loudness_report *d_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = int_probe_refusal(ctx, d_in, src, num_channels, total_frames, h_seg_first_frame, num_segments, lo, hi))
        return rc;
    return loudness_impl(ctx, loudness_source(d_in, src->channel_stride, src->frame_stride, num_segments, num_channels,
                                              src->container_bytes, src->bits, src->left_justified),
                         sample_rate, total_frames, h_seg_first_frame, lo, hi, d_workspace, workspace_bytes, d_energy,
                         energy_rows, d_reports);
}

int32_t alac_hip_loudness_float(alac_hip_ctx *ctx, const float *d_in, uint32_t num_channels, uint64_t channel_stride,
                                uint64_t frame_stride, uint32_t sample_rate, uint64_t total_frames,
                                const uint64_t *h_seg_first_frame, uint32_t num_segments, void *d_workspace,
                                uint64_t workspace_bytes, double *d_energy, uint64_t energy_rows,
                                alac_hip_loudness_report *d_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = float_probe_refusal(ctx, d_in, num_channels, channel_stride, frame_stride, total_frames, h_seg_first_frame,
                                         num_segments, lo, hi))
        return rc;
    return loudness_impl(ctx, loudness_source(d_in, channel_stride, frame_stride, num_segments, num_channels, 0, 0, 0),
                         sample_rate, total_frames, h_seg_first_frame, lo, hi, d_workspace, workspace_bytes, d_energy,
                         energy_rows, d_reports);
}

// ---- true peak: BS.1770-4 annex 2, per segment of frames and channel --------------------------------------------------------
// the workspace: segFirst and chunkBase, [num_segments + 1] each
uint64_t alac_hip_true_peak_workspace_bytes(uint32_t num_channels, uint32_t num_segments)
{
    if (num_channels < 1 || num_channels > kMaxChannels || num_segments == 0) return 0;
    return align_up(2 * ((uint64_t)num_segments + 1) * 8, 256);
}

// What both true-peak calls do behind the source's own refusals (as loudness_impl): the remaining refusals, then the tables to
// the device and the pass.  src: the source (what loudness_source fills).
static int32_t true_peak_impl(alac_hip_ctx *ctx, const LoudArgs &src, uint32_t sample_rate, const uint64_t *h_seg_first_frame,
                              uint64_t lo, uint64_t hi, void *d_workspace, uint64_t workspace_bytes, double *d_channel_peak,
                              void *d_reports)
{
    if (!loud_rate_ok(sample_rate)) return fail(ctx, ALAC_HIP_ParamError, "sample rate is not a multiple of 10 in [8000, 384000]");
    if (!d_reports || ((uintptr_t)d_reports & 7)) return fail(ctx, ALAC_HIP_ParamError, "null or misaligned d_reports (8 B)");
    if (!d_channel_peak || ((uintptr_t)d_channel_peak & 7))
        return fail(ctx, ALAC_HIP_ParamError, "null or misaligned d_channel_peak (8 B)");
    if (!d_workspace || ((uintptr_t)d_workspace & 7)) return fail(ctx, ALAC_HIP_ParamError, "null or misaligned workspace (8 B)");
    const uint32_t nseg = src.numSegments;
    if (workspace_bytes < alac_hip_true_peak_workspace_bytes(src.channels, nseg))
        return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    TruePeakArgs a = {};
    a.in = src.in, a.channelStride = src.channelStride, a.frameStride = src.frameStride;
    a.numSegments = nseg, a.channels = src.channels;
    a.containerBytes = src.containerBytes, a.srcBits = src.srcBits, a.leftJustified = src.leftJustified;
    a.factor = true_peak_factor(sample_rate), a.run = true_peak_run(a.factor);
    std::vector<uint64_t> table(2 * ((size_t)nseg + 1));
    uint64_t *first = table.data(), *chunk = first + nseg + 1;
    chunk[0] = 0;
    for (uint32_t s = 0; s <= nseg; s++) first[s] = h_seg_first_frame ? h_seg_first_frame[s] : (s ? hi : lo);
    for (uint32_t s = 0; s < nseg; s++) chunk[s + 1] = chunk[s] + (first[s + 1] - first[s] + a.run - 1) / a.run;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    hipError_t e;
    if ((e = upload_segment_table(ctx, table.data(), table.size(), d_workspace)))
        return fail(ctx, ALAC_HIP_ParamError, "segment table upload", e);
    a.segFirst = (const uint64_t *)d_workspace, a.chunkBase = a.segFirst + nseg + 1;
    a.totalChunks = chunk[nseg];
    true_peak_coefs(a.factor, a.coef);
    a.channelPeak = (uint64_t *)d_channel_peak;
    a.reports = (uint32_t *)d_reports;
    if ((e = launch_true_peak(a, ctx->stream))) return fail(ctx, ALAC_HIP_ParamError, "true peak launch", e);
    return ALAC_HIP_noErr;
}

int32_t alac_hip_true_peak_int(alac_hip_ctx *ctx, const void *d_in, const alac_hip_int_source *src, uint32_t num_channels,
                               uint32_t sample_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                               uint32_t num_segments, void *d_workspace, uint64_t workspace_bytes, double *d_channel_peak,
                               alac_hip_true_peak_report *d_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = int_probe_refusal(ctx, d_in, src, num_channels, total_frames, h_seg_first_frame, num_segments, lo, hi))
        return rc;
    return true_peak_impl(ctx, loudness_source(d_in, src->channel_stride, src->frame_stride, num_segments, num_channels,
                                               src->container_bytes, src->bits, src->left_justified),
                          sample_rate, h_seg_first_frame, lo, hi, d_workspace, workspace_bytes, d_channel_peak, d_reports);
}

int32_t alac_hip_true_peak_float(alac_hip_ctx *ctx, const float *d_in, uint32_t num_channels, uint64_t channel_stride,
                                 uint64_t frame_stride, uint32_t sample_rate, uint64_t total_frames,
                                 const uint64_t *h_seg_first_frame, uint32_t num_segments, void *d_workspace,
                                 uint64_t workspace_bytes, double *d_channel_peak, alac_hip_true_peak_report *d_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = float_probe_refusal(ctx, d_in, num_channels, channel_stride, frame_stride, total_frames, h_seg_first_frame,
                                         num_segments, lo, hi))
        return rc;
    return true_peak_impl(ctx, loudness_source(d_in, channel_stride, frame_stride, num_segments, num_channels, 0, 0, 0),
                          sample_rate, h_seg_first_frame, lo, hi, d_workspace, workspace_bytes, d_channel_peak, d_reports);
}

// ---- sample-rate conversion: a polyphase windowed-sinc FIR, per segment of frames ---------------------------------------------
// the workspace: segFirst, outFirst and tileBase, [num_segments + 1] each, then the coefficients [L][K]
static uint64_t resample_table_bytes(uint32_t num_segments) { return align_up(3 * ((uint64_t)num_segments + 1) * 8, 256); }

uint64_t alac_hip_resample_workspace_bytes(uint32_t in_rate, uint32_t out_rate, uint32_t num_channels, uint32_t num_segments)
{
    const ResamplePlan p = resample_plan(in_rate, out_rate);
    if (!p.ok || num_channels < 1 || num_channels > kMaxChannels || num_segments == 0) return 0;
    return resample_table_bytes(num_segments) + align_up((uint64_t)p.L * p.K * 8, 256);
}

// What both resampling calls do behind the source's own refusals (as true_peak_impl): the remaining refusals, then the tables
// and the coefficients to the device in one upload, and the pass.  src: the source (what loudness_source fills).
static int32_t resample_impl(alac_hip_ctx *ctx, const LoudArgs &src, uint32_t in_rate, uint32_t out_rate, uint64_t total_frames,
                             const uint64_t *h_seg_first_frame, uint64_t lo, uint64_t hi, void *d_workspace,
                             uint64_t workspace_bytes, float *d_out, uint64_t out_channel_stride, uint64_t out_frames,
                             void *d_reports)
{
    const ResamplePlan p = resample_plan(in_rate, out_rate);
    if (!p.ok)
        return fail(ctx, ALAC_HIP_ParamError,
                    "rates must be different multiples of 10 in [8000, 384000] with L and M of at most 640");
    if (total_frames > UINT64_MAX / 1024) return fail(ctx, ALAC_HIP_ParamError, "total_frames too large");
    if (!d_reports || ((uintptr_t)d_reports & 7)) return fail(ctx, ALAC_HIP_ParamError, "null or misaligned d_reports (8 B)");
    if (!d_out || ((uintptr_t)d_out & 3)) return fail(ctx, ALAC_HIP_ParamError, "null or misaligned d_out (4 B)");
    if (!d_workspace || ((uintptr_t)d_workspace & 15))
        return fail(ctx, ALAC_HIP_ParamError, "null or misaligned workspace (16 B)");
    const uint32_t nseg = src.numSegments;
    if (workspace_bytes < alac_hip_resample_workspace_bytes(in_rate, out_rate, src.channels, nseg))
        return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    ResampleArgs a = {};
    a.in = src.in, a.channelStride = src.channelStride, a.frameStride = src.frameStride;
    a.numSegments = nseg, a.channels = src.channels;
    a.containerBytes = src.containerBytes, a.srcBits = src.srcBits, a.leftJustified = src.leftJustified;
    a.L = p.L, a.M = p.M, a.K = p.K;
    a.tile = resample_tile(p), a.span = (uint32_t)resample_span(p, a.tile);
    const uint64_t tabWords = resample_table_bytes(nseg) / 8, coefWords = (uint64_t)p.L * p.K;
    std::vector<uint64_t> table(tabWords + coefWords, 0);
    uint64_t *first = table.data(), *outFirst = first + nseg + 1, *tileBase = outFirst + nseg + 1;
    for (uint32_t s = 0; s <= nseg; s++) first[s] = h_seg_first_frame ? h_seg_first_frame[s] : (s ? hi : lo);
    for (uint32_t s = 0; s < nseg; s++) {
        const uint64_t n = resample_out_frames(p, first[s + 1] - first[s]);
        outFirst[s + 1] = outFirst[s] + n;
        tileBase[s + 1] = tileBase[s] + (n + a.tile - 1) / a.tile;
    }
    if (out_frames < outFirst[nseg]) return fail(ctx, ALAC_HIP_ParamError, "out_frames below alac_hip_resample_frames");
    if (out_channel_stride < out_frames) return fail(ctx, ALAC_HIP_ParamError, "out_channel_stride below out_frames");
    if (tileBase[nseg] > 0x7fffffffull) return fail(ctx, ALAC_HIP_ParamError, "too many output frames for one call");
    memcpy(table.data() + tabWords, resample_coefs(p) + coefWords, coefWords * 8);  // the kernels' arrangement
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    hipError_t e;
    if ((e = upload_segment_table(ctx, table.data(), table.size(), d_workspace)))
        return fail(ctx, ALAC_HIP_ParamError, "segment table upload", e);
    a.segFirst = (const uint64_t *)d_workspace, a.outFirst = a.segFirst + nseg + 1, a.tileBase = a.outFirst + nseg + 1;
    a.coef = (const double *)(a.segFirst + tabWords);
    a.totalTiles = tileBase[nseg];
    a.out = d_out, a.outChannelStride = out_channel_stride;
    a.reports = (uint32_t *)d_reports;
    if ((e = launch_resample(a, ctx->stream))) return fail(ctx, ALAC_HIP_ParamError, "resample launch", e);
    return ALAC_HIP_noErr;
}

int32_t alac_hip_resample_int(alac_hip_ctx *ctx, const void *d_in, const alac_hip_int_source *src, uint32_t num_channels,
                              uint32_t in_rate, uint32_t out_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                              uint32_t num_segments, void *d_workspace, uint64_t workspace_bytes, float *d_out,
                              uint64_t out_channel_stride, uint64_t out_frames, alac_hip_resample_report *d_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = int_probe_refusal(ctx, d_in, src, num_channels, total_frames, h_seg_first_frame, num_segments, lo, hi))
        return rc;
    return resample_impl(ctx, loudness_source(d_in, src->channel_stride, src->frame_stride, num_segments, num_channels,
                                              src->container_bytes, src->bits, src->left_justified),
                         in_rate, out_rate, total_frames, h_seg_first_frame, lo, hi, d_workspace, workspace_bytes, d_out,
                         out_channel_stride, out_frames, d_reports);
}

int32_t alac_hip_resample_float(alac_hip_ctx *ctx, const float *d_in, uint32_t num_channels, uint64_t channel_stride,
                                uint64_t frame_stride, uint32_t in_rate, uint32_t out_rate, uint64_t total_frames,
                                const uint64_t *h_seg_first_frame, uint32_t num_segments, void *d_workspace,
                                uint64_t workspace_bytes, float *d_out, uint64_t out_channel_stride, uint64_t out_frames,
                                alac_hip_resample_report *d_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = float_probe_refusal(ctx, d_in, num_channels, channel_stride, frame_stride, total_frames, h_seg_first_frame,
                                         num_segments, lo, hi))
        return rc;
    return resample_impl(ctx, loudness_source(d_in, channel_stride, frame_stride, num_segments, num_channels, 0, 0, 0), in_rate,
                         out_rate, total_frames, h_seg_first_frame, lo, hi, d_workspace, workspace_bytes, d_out,
                         out_channel_stride, out_frames, d_reports);
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
    return read_cookie(ck, size, out) ? ALAC_HIP_noErr : ALAC_HIP_ParamError;
}

uint64_t alac_hip_decode_workspace_bytes(const alac_hip_format *fmt, uint32_t num_packets)
{
    return alac_hip_decode_workspace_bytes_stream(fmt, num_packets, 0);
}

uint64_t alac_hip_decode_workspace_bytes_stream(const alac_hip_format *fmt, uint32_t num_packets, uint64_t stream_bytes)
{
    if (!format_ok(fmt)) return 0;
    return dec_layout(fmt, num_packets, stream_bytes).total;
}

}  // extern "C"

namespace {
// ---- decode family: each public call is checked and described once; decode_impl / verify_impl run the description --------
// One call of the ten (five PCM modes, alac_verify.hpp, each in a device and a host form): the format its cookie gives and
// the kernels' arguments.  parse_cookie fills the format's part, a *_mode function the mode's, decode_buffers the buffers.
struct DecodeCall {
    alac_hip_format fmt;
    DecodeArgs da;
    PcmModeArgs pm = {};    // stays empty in the modes whose words fit in `da`
    uint32_t pcmAlign = 4;  // what the mode asks of da.pcmOut's address, in bytes
};

// a call's cookie, parsed once: the format, and into c.da the format's fields and the AG parameters (pb / mb / kb)
int32_t parse_cookie(alac_hip_ctx *ctx, const uint8_t *cookie, uint32_t size, DecodeCall &c)
{
    if (!ctx) return ALAC_HIP_ParamError;
    const uint8_t *ck = read_cookie(cookie, size, &c.fmt);
    if (!ck) return fail(ctx, ALAC_HIP_ParamError, "bad magic cookie");
    if (!format_ok(&c.fmt)) return fail(ctx, ALAC_HIP_ParamError, "unsupported format in cookie");
    c.da.frameSize = c.fmt.frame_size;
    c.da.bitDepth = c.fmt.bit_depth;
    c.da.numChannels = c.fmt.num_channels;
    c.da.pb = ck[6], c.da.mb = ck[7], c.da.kb = ck[8];
    c.da.frameBytes = c.fmt.num_channels * bytes_per_sample(c.fmt.bit_depth);
    return ALAC_HIP_noErr;
}

// The five modes, each from its call's checked arguments.  da.pcmOut is then: store, packed PCM as alac_hip_decode writes it;
// verify, the same, expected and only read; float, planar rows channel_stride floats apart; verify-float, the float source at
// these strides, only read (d_origin: device table, read with dither only); int, containers in the layout of `dst`, aligned
// to their size (int_dest_refusal has checked it).  A host form passes the strides of the compact rows it stages on the device.
void store_mode(DecodeCall &c) { c.da.pcmMode = kPcmStore; }
void verify_mode(DecodeCall &c) { c.da.pcmMode = kPcmVerify; }
void float_mode(DecodeCall &c, uint64_t channel_stride)
{
    c.da.pcmMode = kPcmFloat;
    c.da.channelStride = channel_stride;
}
void verify_float_mode(DecodeCall &c, uint64_t channel_stride, uint64_t frame_stride, const alac_hip_dither *dither,
                       const uint64_t *d_origin)
{
    c.da.pcmMode = kPcmVerifyFloat;
    c.pm.channelStride = channel_stride, c.pm.frameStride = frame_stride;
    c.pm.dither = dither_args(dither, d_origin, c.pm.dz);
}
void int_mode(DecodeCall &c, const alac_hip_int_dest &dst)
{
    c.da.pcmMode = kPcmInt;
    c.pm.channelStride = dst.channel_stride, c.pm.frameStride = dst.frame_stride;
    c.pm.containerBytes = dst.container_bytes;
    c.pm.shift = (dst.left_justified ? 8 * dst.container_bytes : dst.bits) - c.fmt.bit_depth;
    c.pcmAlign = dst.container_bytes == 3 ? 1 : dst.container_bytes;
}

// the device buffers of a call (pcm: see the modes; num_samples_out: null in the verify family, whose counts go to its workspace)
void decode_buffers(DecodeCall &c, const uint8_t *stream, const uint64_t *offsets, uint32_t num_packets, const void *pcm,
                    uint32_t *num_samples_out, int32_t *status)
{
    c.da.stream = stream;
    c.da.offsets = offsets;
    c.da.numPackets = num_packets;
    c.da.pcmOut = (uint8_t *)pcm;
    c.da.numSamplesOut = num_samples_out;
    c.da.statusOut = status;
}

// the decode pass of every decode-family call
int32_t decode_impl(alac_hip_ctx *ctx, const DecodeCall &c, void *d_workspace, uint64_t workspace_bytes)
{
    DecodeArgs da = c.da;  // + the workspace and the context's options
    const uint32_t num_packets = da.numPackets;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!da.stream || !da.offsets || !d_workspace || !da.pcmOut || !da.numSamplesOut || !da.statusOut)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (((uintptr_t)d_workspace & 255) || ((uintptr_t)da.pcmOut & (c.pcmAlign - 1)))
        return fail(ctx, ALAC_HIP_ParamError, "misaligned buffer");
    DecLayout L = dec_layout(&c.fmt, num_packets);
    if (workspace_bytes < L.total) return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    L.capWords = (workspace_bytes - L.words) / 4;  // all of it: packets that do not fit the staged words get status -50
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    // Local hardening, NOT reference behaviour (codec/ag_dec.c:282-286 only checks its pointers; ALACDecoder::Init takes any
    // pb / mb / kb): the kernels shift by kb (k = min(lg3a, kb), m = (1 << k) - 1), so kb outside 1..16 would be an undefined
    // or zero-width shift, and pb = 0 freezes the mean at values the quotient code does not expect.  No encoder writes either.
    if (da.kb < 1 || da.kb > 16 || da.pb == 0) return fail(ctx, ALAC_HIP_ParamError, "bad AG parameters in cookie (pb / kb)");
    uint8_t *ws = (uint8_t *)d_workspace;
    da.maxElems = L.maxElems;
    da.recs = (DecRec *)(ws + L.recs);
    da.resid = (int32_t *)(ws + L.resid);
    da.ho = handoff_ctl(ctx);
    da.optFused = ctx->opt.decFused;
    da.optPair = ctx->opt.decPair;
    da.optDirect = ctx->opt.decDirect;
    hipError_t e;
    if (use_lane_decoder(ctx)) {
        e = launch_decode(da, c.pm, ctx->stream);
    } else if (c.fmt.num_channels > 2) {
        // one pass per element of the channel count's sequence (the position of element k + 1 is only known once
        // element k is entropy-decoded); a stream with another sequence is decoded again by the lane decoder, which
        // follows whatever the packets carry.  This is the one place where the call waits for the GPU.
        McElement el[kMaxChannels];
        const uint32_t nel = channel_elements(c.fmt.num_channels, el);
        e = launch_decode_v1_elements(da, c.pm, el, nel, (uint32_t *)(ws + L.words), L.capWords, da.resid, (uint32_t *)(ws + L.prog),
                                      (uint32_t *)(ws + L.elemBit), (uint32_t *)(ws + L.mismatch), ctx->stream);
        uint32_t mismatch = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&mismatch, ws + L.mismatch, 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess && mismatch) e = launch_decode(da, c.pm, ctx->stream);
    } else {
        // A mono / stereo stream whose packets carry another element sequence (two SCEs for two channels, fill in
        // front of ...: status -4 from the fast pipeline, counted by its header kernel) is decoded again by the lane decoder,
        // which follows whatever the packets carry.  No host round trip: its kernels are gated on that device-side count.
        e = launch_decode_v1(da, c.pm, (uint32_t *)(ws + L.words), L.capWords, da.resid, (uint32_t *)(ws + L.prog), ctx->stream,
                             (uint32_t *)(ws + L.mismatch));
        if (e == hipSuccess) {
            DecodeArgs dg = da;
            dg.gate = (const uint32_t *)(ws + L.mismatch);
            e = launch_decode(dg, c.pm, ctx->stream);
        }
    }
    return e == hipSuccess ? ALAC_HIP_noErr : fail(ctx, ALAC_HIP_ParamError, "decode launch", e);
}

// ---- verify: the decode pass with the PCM store sites comparing against the caller's PCM ----------------------------------
// Workspace: the decoder's own (dec_layout) + the decoded frame counts; no PCM plane on any path — every kernel that writes
// PCM in alac_hip_decode has an instantiation that compares there instead (alac_verify.hpp), the lane decoder's too.
// The decoded frame counts sit in FRONT of the decoder's workspace: the decoder takes everything behind its own layout as
// staging words, so a longer stream only needs a larger workspace here too.
uint64_t verify_ns_bytes(uint32_t numPackets) { return align_up((uint64_t)numPackets * 4, 256); }

// The pass of a call in verify or verify-float mode with the verify family's two device tables.  Verify mode's store sites read
// the first-mismatch table in DecodeArgs, verify-float mode's both tables in the block; each mode leaves the other's place unread.
int32_t verify_impl(alac_hip_ctx *ctx, DecodeCall c, uint32_t *d_first_mismatch, const uint32_t *d_num_samples_expected,
                    void *d_workspace, uint64_t workspace_bytes, uint32_t *d_bad_packets)
{
    DecodeArgs &da = c.da;
    const uint32_t num_packets = da.numPackets;
    da.firstMismatch = c.pm.firstMismatch = d_first_mismatch;
    c.pm.numSamplesExpected = d_num_samples_expected;
    if (!d_bad_packets) return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    if (num_packets == 0) {
        const hipError_t e = hipMemsetAsync(d_bad_packets, 0, 4, ctx->stream);
        return e == hipSuccess ? ALAC_HIP_noErr : fail(ctx, ALAC_HIP_ParamError, "verify launch", e);
    }
    if (!da.stream || !da.offsets || !d_workspace || !da.pcmOut || !d_first_mismatch || !da.statusOut)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (((uintptr_t)d_workspace & 255) || ((uintptr_t)da.pcmOut & (c.pcmAlign - 1)))
        return fail(ctx, ALAC_HIP_ParamError, "misaligned buffer");
    const DecLayout L = dec_layout(&c.fmt, num_packets);
    const uint64_t nsBytes = verify_ns_bytes(num_packets);
    if (workspace_bytes < nsBytes + L.total) return fail(ctx, ALAC_HIP_ParamError, "workspace too small");
    da.numSamplesOut = (uint32_t *)d_workspace;
    hipError_t e = launch_verify_init(d_first_mismatch, num_packets, d_bad_packets, ctx->stream);
    if (e != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "verify launch", e);
    if (int32_t rc = decode_impl(ctx, c, (uint8_t *)d_workspace + nsBytes, workspace_bytes - nsBytes)) return rc;
    e = launch_verify_finish(da.statusOut, da.numSamplesOut, d_num_samples_expected, c.fmt.frame_size, num_packets,
                             d_first_mismatch, d_bad_packets, ctx->stream);
    return e == hipSuccess ? ALAC_HIP_noErr : fail(ctx, ALAC_HIP_ParamError, "verify launch", e);
}

// alac_hip_verify_float's own refusals, device and host form: the dither struct, then (a call with packets) the source
// pointer and the strides by the checks of alac_hip_encode_float
int32_t verify_float_refusal(alac_hip_ctx *ctx, const alac_hip_format &fmt, uint32_t num_packets, const float *in,
                             uint64_t channel_stride, uint64_t frame_stride, const alac_hip_dither *dither,
                             const uint64_t *packet_origin)
{
    if (const char *why = dither_refusal(&fmt, dither, packet_origin)) return fail(ctx, ALAC_HIP_ParamError, why);
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!in) return fail(ctx, ALAC_HIP_ParamError, "null d_in");
    if ((uintptr_t)in & 3) return fail(ctx, ALAC_HIP_ParamError, "misaligned d_in (4 B)");
    return float_stride_refusal(ctx, &fmt, num_packets, channel_stride, frame_stride);
}

// alac_hip_decode_float's refusals of its channel stride, device and host form (a call with packets)
int32_t float_dest_refusal(alac_hip_ctx *ctx, const alac_hip_format &fmt, uint32_t num_packets, uint64_t channel_stride)
{
    if (channel_stride < (uint64_t)num_packets * fmt.frame_size)
        return fail(ctx, ALAC_HIP_ParamError, "channel_stride below num_packets * frame_size");
    if (channel_stride > UINT64_MAX / sizeof(float) / fmt.num_channels)
        return fail(ctx, ALAC_HIP_ParamError, "channel_stride * channels overflows");
    return ALAC_HIP_noErr;
}

// alac_hip_decode_int's own refusals, device and host form (a call with packets): the descriptor by the checks of
// alac_hip_pcm_requantize, the depth, and a layout in which no two samples share a container
int32_t int_dest_refusal(alac_hip_ctx *ctx, const alac_hip_format &fmt, uint32_t num_packets, const void *out,
                         const alac_hip_int_dest *dst)
{
    const uint64_t T = (uint64_t)num_packets * fmt.frame_size, C = fmt.num_channels;
    if (int32_t rc = int_source_struct_refusal(ctx, out, dst, fmt.num_channels, T)) return rc;
    if (dst->bits < fmt.bit_depth)
        return fail(ctx, ALAC_HIP_ParamError, "bits below the stream's depth: alac_hip_decode_int reduces nothing");
    const uint64_t cs = dst->channel_stride, fs = dst->frame_stride;  // fs >= 1; cs >= 1 with more than one channel
    uint64_t need;
    const bool framesInner = !__builtin_mul_overflow(T, fs, &need) && cs >= need;
    const bool channelsInner = !__builtin_mul_overflow(C, cs, &need) && fs >= need;
    if (C > 1 && !framesInner && !channelsInner)
        return fail(ctx, ALAC_HIP_ParamError,
                    "two samples can share a container: neither channel_stride >= num_packets * frame_size * frame_stride "
                    "nor frame_stride >= num_channels * channel_stride");
    return ALAC_HIP_noErr;
}

// The caller's side of a host form: what is staged in and where the results go.  What a mode does not use stays null.
struct HostDecode {
    const uint8_t *stream;
    const uint32_t *packetBytes;
    uint32_t numPackets;
    uint64_t pcmBytes;  // of the PCM side on the device: the rows decoded into, or what is staged of `expected`
    // verify family: the expected PCM / the float source, the expected frame counts and the packets' stream frame indices (both
    // nullable) and the first mismatches (nullable)
    const void *expected = nullptr;
    const uint32_t *numSamplesExpected = nullptr;
    const uint64_t *origin = nullptr;
    uint32_t *firstMismatch = nullptr;
    // decode modes: the PCM and the frame counts; pitch != 0: the PCM as one row per channel, pitch bytes apart
    void *out = nullptr;
    uint64_t pitch = 0;
    uint32_t *numSamplesOut = nullptr;
    int32_t *status = nullptr;  // every mode (nullable in the verify family)
};

// The host forms after their own checks, `c` with its mode set.  Staged: the stream, its workspace, the PCM side (verify
// family: h.expected; else zeroed), the expected frame counts and origins (if given), the statuses.  Then the pass, the copies
// back (decode modes: the PCM and the frame counts; verify family: the first mismatches), the statuses, one wait and the
// hand-off check.  Returns a status, or in the verify family, where all went well, the count of bad packets.
int32_t decode_host_common(alac_hip_ctx *ctx, DecodeCall &c, const HostDecode &h)
{
    const bool verify = c.da.pcmMode == kPcmVerify || c.da.pcmMode == kPcmVerifyFloat;
    const uint32_t num_packets = h.numPackets;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    const uint64_t n4 = num_packets * 4ull;
    hipStream_t st = ctx->stream;
    DevStream d;
    if (int32_t rc = upload_stream(h.stream, h.packetBytes, num_packets, st, d, on_fail(ctx))) return rc;
    const uint64_t wsBytes = (verify ? alac_hip_verify_workspace_bytes_stream : alac_hip_decode_workspace_bytes_stream)(
        &c.fmt, num_packets, d.total);
    DevBuf dWs, dPcm, dNs, dSt, dFm, dBad, dOrigin;
    uint32_t bad = 0;
    hipError_t e;
    if ((e = dWs.alloc(wsBytes)) || (e = dPcm.alloc(h.pcmBytes)) || (e = dNs.alloc(n4)) || (e = dSt.alloc(n4)) ||
        (verify && ((e = dFm.alloc(n4)) || (e = dBad.alloc(4)))) || (h.origin && (e = dOrigin.alloc(num_packets * 8ull))))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if ((h.origin && (e = hipMemcpyAsync(dOrigin.p, h.origin, num_packets * 8ull, hipMemcpyHostToDevice, st))) ||
        (e = verify ? hipMemcpyAsync(dPcm.p, h.expected, h.pcmBytes, hipMemcpyHostToDevice, st)
                    : hipMemsetAsync(dPcm.p, 0, h.pcmBytes, st)) ||
        (h.numSamplesExpected && (e = hipMemcpyAsync(dNs.p, h.numSamplesExpected, n4, hipMemcpyHostToDevice, st))))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    decode_buffers(c, (const uint8_t *)d.bytes.p, (const uint64_t *)d.offs.p, num_packets, dPcm.p, (uint32_t *)dNs.p,
                   (int32_t *)dSt.p);
    if (verify) {
        if (h.origin) c.pm.dz.origin = (const uint64_t *)dOrigin.p;  // the device table the mode could not know yet
        const uint32_t *ns = h.numSamplesExpected ? (const uint32_t *)dNs.p : nullptr;
        if (int32_t rc = verify_impl(ctx, c, (uint32_t *)dFm.p, ns, dWs.p, wsBytes, (uint32_t *)dBad.p)) return rc;
        if (!(e = hipMemcpyAsync(&bad, dBad.p, 4, hipMemcpyDeviceToHost, st)) && h.firstMismatch)
            e = hipMemcpyAsync(h.firstMismatch, dFm.p, n4, hipMemcpyDeviceToHost, st);
    } else {
        if (int32_t rc = decode_impl(ctx, c, dWs.p, wsBytes)) return rc;
        const uint32_t rows = c.fmt.num_channels;
        const uint64_t w = h.pcmBytes / rows;
        if (!(e = h.pitch ? hipMemcpy2DAsync(h.out, h.pitch, dPcm.p, w, w, rows, hipMemcpyDeviceToHost, st)
                          : hipMemcpyAsync(h.out, dPcm.p, h.pcmBytes, hipMemcpyDeviceToHost, st)))
            e = hipMemcpyAsync(h.numSamplesOut, dNs.p, n4, hipMemcpyDeviceToHost, st);
    }
    if (e || (h.status && (e = hipMemcpyAsync(h.status, dSt.p, n4, hipMemcpyDeviceToHost, st))) || (e = hipStreamSynchronize(st)))
        return fail(ctx, ALAC_HIP_ParamError, verify ? "verify execution" : "decode execution", e);
    const int32_t rc = check_handoff(ctx);
    return rc != ALAC_HIP_noErr ? rc : (int32_t)bad;
}
}  // namespace

extern "C" {

int32_t alac_hip_decode(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *d_stream,
                        const uint64_t *d_packet_offsets, uint32_t num_packets, void *d_workspace,
                        uint64_t workspace_bytes, uint8_t *d_pcm_out, uint32_t *d_num_samples_out,
                        int32_t *d_status)
{
    DecodeCall c;
    if (int32_t rc = parse_cookie(ctx, h_cookie, cookie_size, c)) return rc;
    store_mode(c);
    decode_buffers(c, d_stream, d_packet_offsets, num_packets, d_pcm_out, d_num_samples_out, d_status);
    return decode_impl(ctx, c, d_workspace, workspace_bytes);
}

// ---- decode to planar float32: alac_hip_decode with the PCM store sites writing scaled floats ----------------------------
int32_t alac_hip_decode_float(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *d_stream,
                              const uint64_t *d_packet_offsets, uint32_t num_packets, void *d_workspace,
                              uint64_t workspace_bytes, float *d_out, uint64_t channel_stride, uint32_t *d_num_samples_out,
                              int32_t *d_status)
{
    DecodeCall c;
    if (int32_t rc = parse_cookie(ctx, h_cookie, cookie_size, c)) return rc;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!d_out) return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if ((uintptr_t)d_out & 3) return fail(ctx, ALAC_HIP_ParamError, "misaligned buffer");
    if (int32_t rc = float_dest_refusal(ctx, c.fmt, num_packets, channel_stride)) return rc;
    float_mode(c, channel_stride);
    decode_buffers(c, d_stream, d_packet_offsets, num_packets, d_out, d_num_samples_out, d_status);
    return decode_impl(ctx, c, d_workspace, workspace_bytes);
}

// ---- decode to integer containers of any layout: alac_hip_decode with the PCM store sites writing into the caller's layout --
int32_t alac_hip_decode_int(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *d_stream,
                            const uint64_t *d_packet_offsets, uint32_t num_packets, void *d_workspace, uint64_t workspace_bytes,
                            void *d_out, const alac_hip_int_dest *dst, uint32_t *d_num_samples_out, int32_t *d_status)
{
    DecodeCall c;
    if (int32_t rc = parse_cookie(ctx, h_cookie, cookie_size, c)) return rc;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (int32_t rc = int_dest_refusal(ctx, c.fmt, num_packets, d_out, dst)) return rc;
    int_mode(c, *dst);
    decode_buffers(c, d_stream, d_packet_offsets, num_packets, d_out, d_num_samples_out, d_status);
    return decode_impl(ctx, c, d_workspace, workspace_bytes);
}

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
    DecodeCall c;
    if (int32_t rc = parse_cookie(ctx, h_cookie, cookie_size, c)) return rc;
    verify_mode(c);
    decode_buffers(c, d_stream, d_packet_offsets, num_packets, d_pcm_expected, nullptr, d_status);
    return verify_impl(ctx, c, d_first_mismatch, d_num_samples_expected, d_workspace, workspace_bytes, d_bad_packets);
}

// ---- verify against the float32 source of alac_hip_encode_float / _dither: the store sites compare through the rule ----
int32_t alac_hip_verify_float(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *d_stream,
                              const uint64_t *d_packet_offsets, uint32_t num_packets, const float *d_in,
                              uint64_t channel_stride, uint64_t frame_stride, const uint32_t *d_num_samples_expected,
                              const alac_hip_dither *dither, const uint64_t *d_packet_origin, void *d_workspace,
                              uint64_t workspace_bytes, uint32_t *d_first_mismatch, int32_t *d_status, uint32_t *d_bad_packets)
{
    DecodeCall c;
    if (int32_t rc = parse_cookie(ctx, h_cookie, cookie_size, c)) return rc;
    if (int32_t rc = verify_float_refusal(ctx, c.fmt, num_packets, d_in, channel_stride, frame_stride, dither, d_packet_origin))
        return rc;
    verify_float_mode(c, channel_stride, frame_stride, dither, d_packet_origin);
    decode_buffers(c, d_stream, d_packet_offsets, num_packets, d_in, nullptr, d_status);
    return verify_impl(ctx, c, d_first_mismatch, d_num_samples_expected, d_workspace, workspace_bytes, d_bad_packets);
}

// ---- stage level ---------------------------------------------------------------------------------

static int32_t pc_block_any(alac_hip_ctx *ctx, const int32_t *d_in, int32_t *d_out, uint32_t num_rows, uint32_t row_stride,
                            int32_t num, int16_t *d_coefs, int32_t numactive, uint32_t chanbits, uint32_t denshift, bool decode)
{
    if (!ctx || !d_in || !d_out) return ALAC_HIP_ParamError;
    if (numactive < 0 || numactive > 31 || chanbits < 1 || chanbits > 32 || denshift > 15 || num < 0)
        return fail(ctx, ALAC_HIP_ParamError, decode ? "bad unpc_block parameters" : "bad pc_block parameters");
    if (numactive != 0 && numactive != 31 && !d_coefs) return fail(ctx, ALAC_HIP_ParamError, "null coefs");
    hipError_t e = launch_pc_block(d_in, d_out, num_rows, row_stride, num, d_coefs, numactive, chanbits, denshift, decode,
                                   ctx->stream, decode || ctx->opt.stageTaps != 0);
    return e == hipSuccess ? ALAC_HIP_noErr : fail(ctx, ALAC_HIP_ParamError, decode ? "unpc_block launch" : "pc_block launch", e);
}

int32_t alac_hip_pc_block(alac_hip_ctx *ctx, const int32_t *d_in, int32_t *d_pc, uint32_t num_rows,
                          uint32_t row_stride, int32_t num, int16_t *d_coefs, int32_t numactive, uint32_t chanbits,
                          uint32_t denshift)
{
    return pc_block_any(ctx, d_in, d_pc, num_rows, row_stride, num, d_coefs, numactive, chanbits, denshift, false);
}

int32_t alac_hip_unpc_block(alac_hip_ctx *ctx, const int32_t *d_pc, int32_t *d_out, uint32_t num_rows,
                            uint32_t row_stride, int32_t num, int16_t *d_coefs, int32_t numactive,
                            uint32_t chanbits, uint32_t denshift)
{
    return pc_block_any(ctx, d_pc, d_out, num_rows, row_stride, num, d_coefs, numactive, chanbits, denshift, true);
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

// Every host encode form behind its format, source (still the caller's host buffer) and dither.  Staged here: the span of the
// source the call may read, with dither its origin table, for a float or integer source the clip counters; encode_host_common
// stages the rest and the call runs as encode_run, a float or integer source through the stage behind its workspace.
static int32_t encode_host(alac_hip_ctx *ctx, EncodeCall &c, const HostEncode &h)
{
    const alac_hip_format *fmt = &c.fmt;
    const uint32_t np = h.numPackets, nseg = h.numSegments;
    if (h.outTotalBytes) *h.outTotalBytes = 0;
    if (np == 0) return ALAC_HIP_noErr;
    if (!c.src.in || !h.out || !h.packetBytes || !h.numSamples || !h.segFirst || nseg == 0)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (int32_t rc = host_segment_refusal(ctx, h.segFirst, nseg, np)) return rc;
    uint64_t spanBytes = 0;
    if (int32_t rc = source_host_span_bytes(ctx, c.src, fmt, h.numSamples, np, spanBytes)) return rc;
    if (int32_t rc = encode_refusal(ctx, fmt, np, c.lpc ? np : nseg, nullptr, 0, 0)) return rc;
    const bool staged = c.src.kind != SrcKind::Packed, origin = dither_on(c.src.dither) && h.packetOrigin;
    const uint64_t wsBytes =
        (staged ? alac_hip_encode_float_workspace_bytes : alac_hip_encode_workspace_bytes)(fmt, np, c.lpc ? np : nseg);
    const uint64_t encBytes = staged ? (wsBytes - float_stage_bytes(fmt, np)) & ~255ull : wsBytes;
    DevBuf dIn, dClip, dOrigin;
    hipError_t e;
    if ((e = dIn.alloc(spanBytes)) || (staged && (e = dClip.alloc(np * 4ull))) || (origin && (e = dOrigin.alloc(np * 8ull))))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if ((e = hipMemcpyAsync(dIn.p, c.src.in, spanBytes, hipMemcpyHostToDevice, ctx->stream)) ||
        (origin && (e = hipMemcpyAsync(dOrigin.p, h.packetOrigin, np * 8ull, hipMemcpyHostToDevice, ctx->stream))))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    c.src.in = dIn.p, c.src.origin = (const uint64_t *)dOrigin.p, c.src.clipped = h.clipped ? (uint32_t *)dClip.p : nullptr;
    const int32_t rc = encode_host_common(
        ctx->stream, fmt, h, wsBytes,
        [&](const StagedEncode &d) {
            encode_tables(c, d.numSamples, np, d.segFirst, nseg, d.maxSeg);
            encode_state(c, d.state, d.stateIn);
            encode_buffers(c, d.ws, d.out, d.packetBytes, d.offsets);
            encode_pcm(c, encBytes);
            return encode_run(ctx, c);
        },
        on_fail(ctx), [ctx] { return alac_hip_synchronize(ctx); });
    if (rc != ALAC_HIP_noErr || !h.clipped) return rc;
    if ((e = hipMemcpyAsync(h.clipped, dClip.p, np * 4ull, hipMemcpyDeviceToHost, ctx->stream)) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "D2H copy", e);
    return ALAC_HIP_noErr;
}

int32_t alac_hip_encode_host_segments(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *h_pcm,
                                      const uint32_t *h_num_samples, uint32_t num_packets, const uint32_t *h_seg_first,
                                      uint32_t num_segments, int16_t *h_state, int32_t state_in, uint8_t *h_out,
                                      uint64_t out_capacity, uint32_t *h_packet_bytes, uint64_t *out_total_bytes)
{
    EncodeCall c;
    if (int32_t rc = encode_format(ctx, fmt, packed_source(h_pcm), c)) return rc;
    return encode_host(ctx, c, {h_num_samples, num_packets, h_seg_first, num_segments, h_state, state_in, h_out, out_capacity,
                                h_packet_bytes, out_total_bytes});
}

int32_t alac_hip_encode_float_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const float *h_in, uint64_t channel_stride,
                                   uint64_t frame_stride, const uint32_t *h_num_samples, uint32_t num_packets,
                                   const uint32_t *h_seg_first, uint32_t num_segments, int16_t *h_state, int32_t state_in,
                                   uint8_t *h_out, uint64_t out_capacity, uint32_t *h_packet_bytes, uint64_t *out_total_bytes,
                                   uint32_t *h_clipped)
{
    return alac_hip_encode_float_dither_host(ctx, fmt, h_in, channel_stride, frame_stride, h_num_samples, num_packets,
                                             h_seg_first, num_segments, h_state, state_in, h_out, out_capacity, h_packet_bytes,
                                             out_total_bytes, h_clipped, nullptr, nullptr);
}

int32_t alac_hip_encode_float_dither_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const float *h_in,
                                          uint64_t channel_stride, uint64_t frame_stride, const uint32_t *h_num_samples,
                                          uint32_t num_packets, const uint32_t *h_seg_first, uint32_t num_segments,
                                          int16_t *h_state, int32_t state_in, uint8_t *h_out, uint64_t out_capacity,
                                          uint32_t *h_packet_bytes, uint64_t *out_total_bytes, uint32_t *h_clipped,
                                          const alac_hip_dither *dither, const uint64_t *h_packet_origin)
{
    EncodeCall c;
    if (int32_t rc = encode_format(ctx, fmt, float_source(h_in, channel_stride, frame_stride), c)) return rc;
    if (int32_t rc = source_dither(ctx, fmt, c.src, dither, h_packet_origin, nullptr)) return rc;
    return encode_host(ctx, c, {h_num_samples, num_packets, h_seg_first, num_segments, h_state, state_in, h_out, out_capacity,
                                h_packet_bytes, out_total_bytes, h_clipped, h_packet_origin});
}

int32_t alac_hip_pcm_requantize_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *h_in,
                                     const alac_hip_int_source *src, const uint32_t *h_num_samples, uint32_t num_packets,
                                     uint8_t *h_pcm_out, uint64_t pcm_capacity, uint32_t *h_clipped,
                                     const alac_hip_dither *dither, const uint64_t *h_packet_origin)
{
    if (!ctx) return ALAC_HIP_ParamError;
    if (!format_ok(fmt)) return fail(ctx, ALAC_HIP_ParamError, "unsupported format");
    EncodeSource s = int_source(h_in, src);
    if (int32_t rc = source_dither(ctx, fmt, s, dither, h_packet_origin, nullptr)) return rc;
    if (num_packets == 0) return ALAC_HIP_noErr;
    uint64_t spanBytes = 0;
    if (int32_t rc = source_host_span_bytes(ctx, s, fmt, h_num_samples, num_packets, spanBytes)) return rc;
    const uint32_t np = num_packets;
    const uint64_t pcmBytes = packed_pcm_bytes(fmt, np);
    if (!h_pcm_out) return fail(ctx, ALAC_HIP_ParamError, "null h_pcm_out");
    if (pcm_capacity < pcmBytes) return fail(ctx, ALAC_HIP_ParamError, "pcm_capacity below num_packets packets");
    const bool origin = dither_on(dither) && h_packet_origin;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    DevBuf dIn, dNs, dPcm, dClip, dOrigin;
    hipError_t e;
    if ((e = dIn.alloc(spanBytes)) || (h_num_samples && (e = dNs.alloc(np * 4ull))) || (e = dPcm.alloc(pcmBytes)) ||
        (e = dClip.alloc(np * 4ull)) || (origin && (e = dOrigin.alloc(np * 8ull))))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if ((e = hipMemcpyAsync(dIn.p, h_in, spanBytes, hipMemcpyHostToDevice, ctx->stream)) ||
        (h_num_samples && (e = hipMemcpyAsync(dNs.p, h_num_samples, np * 4ull, hipMemcpyHostToDevice, ctx->stream))) ||
        (origin && (e = hipMemcpyAsync(dOrigin.p, h_packet_origin, np * 8ull, hipMemcpyHostToDevice, ctx->stream))))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    s.in = dIn.p, s.origin = (const uint64_t *)dOrigin.p, s.clipped = h_clipped ? (uint32_t *)dClip.p : nullptr;
    if (int32_t rc = source_convert(ctx, s, *fmt, ctx->stream, (const uint32_t *)dNs.p, np, dPcm.p)) return rc;
    if ((e = hipMemcpyAsync(h_pcm_out, dPcm.p, pcmBytes, hipMemcpyDeviceToHost, ctx->stream)) ||
        (h_clipped && (e = hipMemcpyAsync(h_clipped, dClip.p, np * 4ull, hipMemcpyDeviceToHost, ctx->stream))) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "D2H copy", e);
    return ALAC_HIP_noErr;
}

int32_t alac_hip_encode_int_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *h_in, const alac_hip_int_source *src,
                                 const uint32_t *h_num_samples, uint32_t num_packets, const uint32_t *h_seg_first,
                                 uint32_t num_segments, int16_t *h_state, int32_t state_in, uint8_t *h_out,
                                 uint64_t out_capacity, uint32_t *h_packet_bytes, uint64_t *out_total_bytes,
                                 uint32_t *h_clipped, const alac_hip_dither *dither, const uint64_t *h_packet_origin)
{
    EncodeCall c;
    if (int32_t rc = encode_format(ctx, fmt, int_source(h_in, src), c)) return rc;
    if (int32_t rc = source_dither(ctx, fmt, c.src, dither, h_packet_origin, nullptr)) return rc;
    return encode_host(ctx, c, {h_num_samples, num_packets, h_seg_first, num_segments, h_state, state_in, h_out, out_capacity,
                                h_packet_bytes, out_total_bytes, h_clipped, h_packet_origin});
}

int32_t alac_hip_float_probe_host(alac_hip_ctx *ctx, const float *h_in, uint32_t num_channels, uint64_t channel_stride,
                                  uint64_t frame_stride, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                  uint32_t num_segments, alac_hip_float_report *h_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = float_probe_refusal(ctx, h_in, num_channels, channel_stride, frame_stride, total_frames, h_seg_first_frame,
                                         num_segments, lo, hi))
        return rc;
    if (!h_reports) return fail(ctx, ALAC_HIP_ParamError, "null h_reports");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    // the floats the call may read lie in [0, span) of h_in: up to the last frame of the last segment
    const uint64_t span = hi > lo ? (num_channels - 1) * channel_stride + (hi - 1) * frame_stride + 1 : 0;
    const uint64_t wsBytes = alac_hip_float_probe_workspace_bytes(num_segments), repBytes = (uint64_t)num_segments * 32;
    DevBuf dIn, dWs, dRep;
    hipError_t e;
    if ((e = dIn.alloc(span * sizeof(float))) || (e = dWs.alloc(wsBytes)) || (e = dRep.alloc(repBytes)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if (span && (e = hipMemcpyAsync(dIn.p, h_in, span * sizeof(float), hipMemcpyHostToDevice, ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    if (int32_t rc = alac_hip_float_probe(ctx, (const float *)dIn.p, num_channels, channel_stride, frame_stride, total_frames,
                                          h_seg_first_frame, num_segments, dWs.p, wsBytes, (alac_hip_float_report *)dRep.p))
        return rc;
    if ((e = hipMemcpyAsync(h_reports, dRep.p, repBytes, hipMemcpyDeviceToHost, ctx->stream)) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "D2H copy", e);
    return ALAC_HIP_noErr;
}

int32_t alac_hip_int_probe_host(alac_hip_ctx *ctx, const void *h_in, const alac_hip_int_source *src, uint32_t num_channels,
                                uint64_t total_frames, const uint64_t *h_seg_first_frame, uint32_t num_segments,
                                alac_hip_int_report *h_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = int_probe_refusal(ctx, h_in, src, num_channels, total_frames, h_seg_first_frame, num_segments, lo, hi))
        return rc;
    if (!h_reports) return fail(ctx, ALAC_HIP_ParamError, "null h_reports");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    // the containers the call may read lie in [0, span) of h_in: up to the last frame of the last segment
    const uint64_t span = hi > lo ? (num_channels - 1) * src->channel_stride + (hi - 1) * src->frame_stride + 1 : 0;
    const uint64_t spanBytes = span * src->container_bytes;
    const uint64_t wsBytes = alac_hip_int_probe_workspace_bytes(num_segments), repBytes = (uint64_t)num_segments * 32;
    DevBuf dIn, dWs, dRep;
    hipError_t e;
    if ((e = dIn.alloc(spanBytes)) || (e = dWs.alloc(wsBytes)) || (e = dRep.alloc(repBytes)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if (spanBytes && (e = hipMemcpyAsync(dIn.p, h_in, spanBytes, hipMemcpyHostToDevice, ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    if (int32_t rc = alac_hip_int_probe(ctx, dIn.p, src, num_channels, total_frames, h_seg_first_frame, num_segments, dWs.p,
                                        wsBytes, (alac_hip_int_report *)dRep.p))
        return rc;
    if ((e = hipMemcpyAsync(h_reports, dRep.p, repBytes, hipMemcpyDeviceToHost, ctx->stream)) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "D2H copy", e);
    return ALAC_HIP_noErr;
}

extern "C++" {
// the host form of a loudness call whose source refusals have passed: stages spanBytes of h_in, runs call(d_in, workspace,
// its bytes, d_energy, d_reports), brings the table's rows and the reports back
template <typename Call>
static int32_t loudness_host(alac_hip_ctx *ctx, const void *h_in, uint64_t spanBytes, uint32_t num_channels, uint32_t sample_rate,
                             uint64_t total_frames, const uint64_t *h_seg_first_frame, uint32_t num_segments, double *h_energy,
                             uint64_t energy_rows, alac_hip_loudness_report *h_reports, Call call)
{
    if (!h_reports || !h_energy) return fail(ctx, ALAC_HIP_ParamError, "null h_energy or h_reports");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    const uint64_t rows = alac_hip_loudness_rows(sample_rate, total_frames, h_seg_first_frame, num_segments);
    if (energy_rows < rows) return fail(ctx, ALAC_HIP_ParamError, "energy_rows below the table's row count");
    const uint64_t wsBytes = alac_hip_loudness_workspace_bytes(sample_rate, num_channels, total_frames, num_segments);
    const uint64_t rowBytes = rows * num_channels * 8, repBytes = (uint64_t)num_segments * 32;
    DevBuf dIn, dWs, dRows, dRep;
    hipError_t e;
    if ((e = dIn.alloc(spanBytes)) || (e = dWs.alloc(wsBytes)) || (e = dRows.alloc(rowBytes)) || (e = dRep.alloc(repBytes)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if (spanBytes && (e = hipMemcpyAsync(dIn.p, h_in, spanBytes, hipMemcpyHostToDevice, ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    if (int32_t rc = call(dIn.p, dWs.p, wsBytes, (double *)dRows.p, rows, (alac_hip_loudness_report *)dRep.p)) return rc;
    if ((rowBytes && (e = hipMemcpyAsync(h_energy, dRows.p, rowBytes, hipMemcpyDeviceToHost, ctx->stream))) ||
        (e = hipMemcpyAsync(h_reports, dRep.p, repBytes, hipMemcpyDeviceToHost, ctx->stream)) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "D2H copy", e);
    return ALAC_HIP_noErr;
}

}  // extern "C++"

int32_t alac_hip_loudness_int_host(alac_hip_ctx *ctx, const void *h_in, const alac_hip_int_source *src, uint32_t num_channels,
                                   uint32_t sample_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                   uint32_t num_segments, double *h_energy, uint64_t energy_rows,
                                   alac_hip_loudness_report *h_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = int_probe_refusal(ctx, h_in, src, num_channels, total_frames, h_seg_first_frame, num_segments, lo, hi))
        return rc;
    if (!loud_rate_ok(sample_rate)) return fail(ctx, ALAC_HIP_ParamError, "sample rate is not a multiple of 10 in [8000, 384000]");
    // the containers the call may read lie in [0, span) of h_in: up to the last frame of the last segment
    const uint64_t span = hi > lo ? (num_channels - 1) * src->channel_stride + (hi - 1) * src->frame_stride + 1 : 0;
    return loudness_host(ctx, h_in, span * src->container_bytes, num_channels, sample_rate, total_frames, h_seg_first_frame,
                         num_segments, h_energy, energy_rows, h_reports,
                         [&](void *dIn, void *dWs, uint64_t wsBytes, double *dRows, uint64_t rows, alac_hip_loudness_report *dRep) {
                             return alac_hip_loudness_int(ctx, dIn, src, num_channels, sample_rate, total_frames,
                                                          h_seg_first_frame, num_segments, dWs, wsBytes, dRows, rows, dRep);
                         });
}

int32_t alac_hip_loudness_float_host(alac_hip_ctx *ctx, const float *h_in, uint32_t num_channels, uint64_t channel_stride,
                                     uint64_t frame_stride, uint32_t sample_rate, uint64_t total_frames,
                                     const uint64_t *h_seg_first_frame, uint32_t num_segments, double *h_energy,
                                     uint64_t energy_rows, alac_hip_loudness_report *h_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = float_probe_refusal(ctx, h_in, num_channels, channel_stride, frame_stride, total_frames, h_seg_first_frame,
                                         num_segments, lo, hi))
        return rc;
    if (!loud_rate_ok(sample_rate)) return fail(ctx, ALAC_HIP_ParamError, "sample rate is not a multiple of 10 in [8000, 384000]");
    const uint64_t span = hi > lo ? (num_channels - 1) * channel_stride + (hi - 1) * frame_stride + 1 : 0;
    return loudness_host(ctx, h_in, span * sizeof(float), num_channels, sample_rate, total_frames, h_seg_first_frame,
                         num_segments, h_energy, energy_rows, h_reports,
                         [&](void *dIn, void *dWs, uint64_t wsBytes, double *dRows, uint64_t rows, alac_hip_loudness_report *dRep) {
                             return alac_hip_loudness_float(ctx, (const float *)dIn, num_channels, channel_stride, frame_stride,
                                                            sample_rate, total_frames, h_seg_first_frame, num_segments, dWs,
                                                            wsBytes, dRows, rows, dRep);
                         });
}

extern "C++" {
// the host form of a true-peak call whose source refusals have passed, as loudness_host: stages spanBytes of h_in, runs
// call(d_in, workspace, its bytes, d_channel_peak, d_reports), brings the channel peaks and the reports back
template <typename Call>
static int32_t true_peak_host(alac_hip_ctx *ctx, const void *h_in, uint64_t spanBytes, uint32_t num_channels,
                              uint32_t num_segments, double *h_channel_peak, alac_hip_true_peak_report *h_reports, Call call)
{
    if (!h_reports || !h_channel_peak) return fail(ctx, ALAC_HIP_ParamError, "null h_channel_peak or h_reports");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    const uint64_t wsBytes = alac_hip_true_peak_workspace_bytes(num_channels, num_segments);
    const uint64_t peakBytes = (uint64_t)num_segments * num_channels * 8, repBytes = (uint64_t)num_segments * 32;
    DevBuf dIn, dWs, dPeak, dRep;
    hipError_t e;
    if ((e = dIn.alloc(spanBytes)) || (e = dWs.alloc(wsBytes)) || (e = dPeak.alloc(peakBytes)) || (e = dRep.alloc(repBytes)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if (spanBytes && (e = hipMemcpyAsync(dIn.p, h_in, spanBytes, hipMemcpyHostToDevice, ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    if (int32_t rc = call(dIn.p, dWs.p, wsBytes, (double *)dPeak.p, (alac_hip_true_peak_report *)dRep.p)) return rc;
    if ((e = hipMemcpyAsync(h_channel_peak, dPeak.p, peakBytes, hipMemcpyDeviceToHost, ctx->stream)) ||
        (e = hipMemcpyAsync(h_reports, dRep.p, repBytes, hipMemcpyDeviceToHost, ctx->stream)) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "D2H copy", e);
    return ALAC_HIP_noErr;
}

}  // extern "C++"

int32_t alac_hip_true_peak_int_host(alac_hip_ctx *ctx, const void *h_in, const alac_hip_int_source *src, uint32_t num_channels,
                                    uint32_t sample_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                    uint32_t num_segments, double *h_channel_peak, alac_hip_true_peak_report *h_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = int_probe_refusal(ctx, h_in, src, num_channels, total_frames, h_seg_first_frame, num_segments, lo, hi))
        return rc;
    if (!loud_rate_ok(sample_rate)) return fail(ctx, ALAC_HIP_ParamError, "sample rate is not a multiple of 10 in [8000, 384000]");
    // the containers the call may read lie in [0, span) of h_in: up to the last frame of the last segment
    const uint64_t span = hi > lo ? (num_channels - 1) * src->channel_stride + (hi - 1) * src->frame_stride + 1 : 0;
    return true_peak_host(ctx, h_in, span * src->container_bytes, num_channels, num_segments, h_channel_peak, h_reports,
                          [&](void *dIn, void *dWs, uint64_t wsBytes, double *dPeak, alac_hip_true_peak_report *dRep) {
                              return alac_hip_true_peak_int(ctx, dIn, src, num_channels, sample_rate, total_frames,
                                                            h_seg_first_frame, num_segments, dWs, wsBytes, dPeak, dRep);
                          });
}

int32_t alac_hip_true_peak_float_host(alac_hip_ctx *ctx, const float *h_in, uint32_t num_channels, uint64_t channel_stride,
                                      uint64_t frame_stride, uint32_t sample_rate, uint64_t total_frames,
                                      const uint64_t *h_seg_first_frame, uint32_t num_segments, double *h_channel_peak,
                                      alac_hip_true_peak_report *h_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = float_probe_refusal(ctx, h_in, num_channels, channel_stride, frame_stride, total_frames, h_seg_first_frame,
                                         num_segments, lo, hi))
        return rc;
    if (!loud_rate_ok(sample_rate)) return fail(ctx, ALAC_HIP_ParamError, "sample rate is not a multiple of 10 in [8000, 384000]");
    const uint64_t span = hi > lo ? (num_channels - 1) * channel_stride + (hi - 1) * frame_stride + 1 : 0;
    return true_peak_host(ctx, h_in, span * sizeof(float), num_channels, num_segments, h_channel_peak, h_reports,
                          [&](void *dIn, void *dWs, uint64_t wsBytes, double *dPeak, alac_hip_true_peak_report *dRep) {
                              return alac_hip_true_peak_float(ctx, (const float *)dIn, num_channels, channel_stride,
                                                              frame_stride, sample_rate, total_frames, h_seg_first_frame,
                                                              num_segments, dWs, wsBytes, dPeak, dRep);
                          });
}

extern "C++" {
// the host form of a resampling call whose source refusals have passed, as true_peak_host: stages spanBytes of h_in, runs
// call(d_in, workspace, its bytes, d_out, d_reports) with the rows out_frames apart, brings the rows (to h_out, out_channel_stride
// apart) and the reports back
template <typename Call>
static int32_t resample_host(alac_hip_ctx *ctx, const void *h_in, uint64_t spanBytes, uint32_t in_rate, uint32_t out_rate,
                             uint32_t num_channels, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                             uint32_t num_segments, float *h_out, uint64_t out_channel_stride, uint64_t out_frames,
                             alac_hip_resample_report *h_reports, Call call)
{
    if (!h_reports || !h_out) return fail(ctx, ALAC_HIP_ParamError, "null h_out or h_reports");
    const uint64_t wsBytes = alac_hip_resample_workspace_bytes(in_rate, out_rate, num_channels, num_segments);
    if (!wsBytes)
        return fail(ctx, ALAC_HIP_ParamError,
                    "rates must be different multiples of 10 in [8000, 384000] with L and M of at most 640");
    const uint64_t total = alac_hip_resample_frames(in_rate, out_rate, total_frames, h_seg_first_frame, num_segments, nullptr);
    if (out_frames < total) return fail(ctx, ALAC_HIP_ParamError, "out_frames below alac_hip_resample_frames");
    if (out_channel_stride < out_frames) return fail(ctx, ALAC_HIP_ParamError, "out_channel_stride below out_frames");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    const uint64_t repBytes = (uint64_t)num_segments * 32;
    DevBuf dIn, dWs, dOut, dRep;
    hipError_t e;
    if ((e = dIn.alloc(spanBytes)) || (e = dWs.alloc(wsBytes)) || (e = dOut.alloc((uint64_t)num_channels * total * 4)) ||
        (e = dRep.alloc(repBytes)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if (spanBytes && (e = hipMemcpyAsync(dIn.p, h_in, spanBytes, hipMemcpyHostToDevice, ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    if (int32_t rc = call(dIn.p, dWs.p, wsBytes, (float *)dOut.p, total, (alac_hip_resample_report *)dRep.p)) return rc;
    for (uint32_t c = 0; c < num_channels && total; c++)
        if ((e = hipMemcpyAsync(h_out + c * out_channel_stride, (const float *)dOut.p + c * total, total * 4,
                                hipMemcpyDeviceToHost, ctx->stream)))
            return fail(ctx, ALAC_HIP_ParamError, "D2H copy", e);
    if ((e = hipMemcpyAsync(h_reports, dRep.p, repBytes, hipMemcpyDeviceToHost, ctx->stream)) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "D2H copy", e);
    return ALAC_HIP_noErr;
}

}  // extern "C++"

int32_t alac_hip_resample_int_host(alac_hip_ctx *ctx, const void *h_in, const alac_hip_int_source *src, uint32_t num_channels,
                                   uint32_t in_rate, uint32_t out_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                   uint32_t num_segments, float *h_out, uint64_t out_channel_stride, uint64_t out_frames,
                                   alac_hip_resample_report *h_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = int_probe_refusal(ctx, h_in, src, num_channels, total_frames, h_seg_first_frame, num_segments, lo, hi))
        return rc;
    // the containers the call may read lie in [0, span) of h_in: up to the last frame of the last segment
    const uint64_t span = hi > lo ? (num_channels - 1) * src->channel_stride + (hi - 1) * src->frame_stride + 1 : 0;
    return resample_host(ctx, h_in, span * src->container_bytes, in_rate, out_rate, num_channels, total_frames,
                         h_seg_first_frame, num_segments, h_out, out_channel_stride, out_frames, h_reports,
                         [&](void *dIn, void *dWs, uint64_t wsBytes, float *dOut, uint64_t total, alac_hip_resample_report *dRep) {
                             return alac_hip_resample_int(ctx, dIn, src, num_channels, in_rate, out_rate, total_frames,
                                                          h_seg_first_frame, num_segments, dWs, wsBytes, dOut, total, total, dRep);
                         });
}

int32_t alac_hip_resample_float_host(alac_hip_ctx *ctx, const float *h_in, uint32_t num_channels, uint64_t channel_stride,
                                     uint64_t frame_stride, uint32_t in_rate, uint32_t out_rate, uint64_t total_frames,
                                     const uint64_t *h_seg_first_frame, uint32_t num_segments, float *h_out,
                                     uint64_t out_channel_stride, uint64_t out_frames, alac_hip_resample_report *h_reports)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = float_probe_refusal(ctx, h_in, num_channels, channel_stride, frame_stride, total_frames, h_seg_first_frame,
                                         num_segments, lo, hi))
        return rc;
    const uint64_t span = hi > lo ? (num_channels - 1) * channel_stride + (hi - 1) * frame_stride + 1 : 0;
    return resample_host(ctx, h_in, span * sizeof(float), in_rate, out_rate, num_channels, total_frames, h_seg_first_frame,
                         num_segments, h_out, out_channel_stride, out_frames, h_reports,
                         [&](void *dIn, void *dWs, uint64_t wsBytes, float *dOut, uint64_t total, alac_hip_resample_report *dRep) {
                             return alac_hip_resample_float(ctx, (const float *)dIn, num_channels, channel_stride, frame_stride,
                                                            in_rate, out_rate, total_frames, h_seg_first_frame, num_segments, dWs,
                                                            wsBytes, dOut, total, total, dRep);
                         });
}

int32_t alac_hip_pcm_crc32_host(alac_hip_ctx *ctx, const void *h_pcm, uint64_t total_bytes, const uint64_t *h_ranges,
                                uint32_t num_ranges, alac_hip_pcm_digest *h_digests)
{
    if (!ctx) return ALAC_HIP_ParamError;
    uint64_t lo, hi;
    if (int32_t rc = pcm_crc_refusal(ctx, h_pcm, total_bytes, h_ranges, num_ranges, lo, hi)) return rc;
    if (!h_digests) return fail(ctx, ALAC_HIP_ParamError, "null h_digests");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, ALAC_HIP_ParamError, "hipSetDevice");
    // the bytes the call may read lie in [0, hi) of h_pcm: up to the last range's end
    const uint64_t wsBytes = h_ranges ? alac_hip_pcm_crc32_workspace_bytes(num_ranges) : 0, digBytes = (uint64_t)num_ranges * 16;
    DevBuf dPcm, dWs, dDig;
    hipError_t e;
    if ((e = dPcm.alloc(hi)) || (e = dWs.alloc(wsBytes)) || (e = dDig.alloc(digBytes)))
        return fail(ctx, ALAC_HIP_MemFullError, "hipMalloc", e);
    if (hi && (e = hipMemcpyAsync(dPcm.p, h_pcm, hi, hipMemcpyHostToDevice, ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "H2D copy", e);
    if (int32_t rc = alac_hip_pcm_crc32(ctx, dPcm.p, hi, h_ranges, num_ranges, dWs.p, wsBytes, (alac_hip_pcm_digest *)dDig.p))
        return rc;
    if ((e = hipMemcpyAsync(h_digests, dDig.p, digBytes, hipMemcpyDeviceToHost, ctx->stream)) ||
        (e = hipStreamSynchronize(ctx->stream)))
        return fail(ctx, ALAC_HIP_ParamError, "D2H copy", e);
    return ALAC_HIP_noErr;
}

int32_t alac_hip_encode_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *h_pcm,
                             uint64_t total_samples, uint32_t segment_packets, int16_t *h_state, int32_t state_in,
                             uint8_t *h_out, uint64_t out_capacity, uint32_t *h_packet_bytes,
                             uint64_t *out_total_bytes)
{
    EncodeCall c;
    if (int32_t rc = encode_format(ctx, fmt, packed_source(h_pcm), c)) return rc;
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
    std::vector<uint8_t> padded;
    if (inBytes != pcmBytes) {
        padded.assign(pcmBytes, 0);
        memcpy(padded.data(), h_pcm, inBytes);
        c.src.in = padded.data();
    }
    return encode_host(ctx, c, {ns.data(), np, segFirst.data(), nseg, h_state, state_in, h_out, out_capacity, h_packet_bytes,
                                out_total_bytes});
}

int32_t alac_hip_decode_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size,
                             const uint8_t *h_stream, const uint32_t *h_packet_bytes, uint32_t num_packets,
                             uint8_t *h_pcm_out, uint32_t *h_num_samples_out, int32_t *h_status)
{
    DecodeCall c;
    if (int32_t rc = parse_cookie(ctx, h_cookie, cookie_size, c)) return rc;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!h_stream || !h_packet_bytes || !h_pcm_out || !h_num_samples_out || !h_status)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    store_mode(c);
    HostDecode h{h_stream, h_packet_bytes, num_packets, packed_pcm_bytes(&c.fmt, num_packets)};
    h.out = h_pcm_out, h.numSamplesOut = h_num_samples_out, h.status = h_status;
    return decode_host_common(ctx, c, h);
}

int32_t alac_hip_decode_float_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size,
                                   const uint8_t *h_stream, const uint32_t *h_packet_bytes, uint32_t num_packets, float *h_out,
                                   uint64_t channel_stride, uint32_t *h_num_samples_out, int32_t *h_status)
{
    DecodeCall c;
    if (int32_t rc = parse_cookie(ctx, h_cookie, cookie_size, c)) return rc;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!h_stream || !h_packet_bytes || !h_out || !h_num_samples_out || !h_status)
        return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (int32_t rc = float_dest_refusal(ctx, c.fmt, num_packets, channel_stride)) return rc;
    // on the device the rows lie back to back; the copy back puts them channel_stride floats apart and leaves the gap alone
    const uint64_t row = (uint64_t)num_packets * c.fmt.frame_size;  // floats of one channel
    float_mode(c, row);
    HostDecode h{h_stream, h_packet_bytes, num_packets, row * c.fmt.num_channels * sizeof(float)};
    h.out = h_out, h.pitch = channel_stride * sizeof(float), h.numSamplesOut = h_num_samples_out, h.status = h_status;
    return decode_host_common(ctx, c, h);
}

int32_t alac_hip_decode_int_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *h_stream,
                                 const uint32_t *h_packet_bytes, uint32_t num_packets, void *h_out, const alac_hip_int_dest *dst,
                                 uint32_t *h_num_samples_out, int32_t *h_status)
{
    DecodeCall c;
    if (int32_t rc = parse_cookie(ctx, h_cookie, cookie_size, c)) return rc;
    if (num_packets == 0) return ALAC_HIP_noErr;
    if (!h_stream || !h_packet_bytes || !h_num_samples_out || !h_status) return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (int32_t rc = int_dest_refusal(ctx, c.fmt, num_packets, h_out, dst)) return rc;
    // on the device the containers lie as planar rows back to back; the host puts each at the caller's index and leaves the
    // bytes between containers alone
    const uint64_t T = (uint64_t)num_packets * c.fmt.frame_size;
    const uint32_t cb = dst->container_bytes;
    alac_hip_int_dest rows = *dst;
    rows.frame_stride = 1;
    rows.channel_stride = T;
    int_mode(c, rows);
    std::vector<uint8_t> stage(T * c.fmt.num_channels * cb);
    HostDecode h{h_stream, h_packet_bytes, num_packets, stage.size()};
    h.out = stage.data(), h.numSamplesOut = h_num_samples_out, h.status = h_status;
    if (int32_t rc = decode_host_common(ctx, c, h)) return rc;
    const uint8_t *from = stage.data();
    for (uint32_t ch = 0; ch < c.fmt.num_channels; ch++)
        for (uint64_t t = 0; t < T; t++, from += cb)
            memcpy((uint8_t *)h_out + (ch * dst->channel_stride + t * dst->frame_stride) * cb, from, cb);
    return ALAC_HIP_noErr;
}

int32_t alac_hip_verify_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *h_stream,
                             const uint32_t *h_packet_bytes, uint32_t num_packets, const uint8_t *h_pcm_expected,
                             const uint32_t *h_num_samples_expected, uint32_t *h_first_mismatch, int32_t *h_status)
{
    DecodeCall c;
    if (int32_t rc = parse_cookie(ctx, h_cookie, cookie_size, c)) return rc;
    if (num_packets == 0) return 0;
    if (!h_stream || !h_packet_bytes || !h_pcm_expected) return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (num_packets > 0x7fffffffu) return fail(ctx, ALAC_HIP_ParamError, "more packets than the return value counts");
    verify_mode(c);
    HostDecode h{h_stream, h_packet_bytes, num_packets, packed_pcm_bytes(&c.fmt, num_packets)};
    h.expected = h_pcm_expected, h.numSamplesExpected = h_num_samples_expected;
    h.firstMismatch = h_first_mismatch, h.status = h_status;
    return decode_host_common(ctx, c, h);
}

int32_t alac_hip_verify_float_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *h_stream,
                                   const uint32_t *h_packet_bytes, uint32_t num_packets, const float *h_in,
                                   uint64_t channel_stride, uint64_t frame_stride, const uint32_t *h_num_samples_expected,
                                   const alac_hip_dither *dither, const uint64_t *h_packet_origin, uint32_t *h_first_mismatch,
                                   int32_t *h_status)
{
    DecodeCall c;
    if (int32_t rc = parse_cookie(ctx, h_cookie, cookie_size, c)) return rc;
    if (int32_t rc = verify_float_refusal(ctx, c.fmt, num_packets, h_in, channel_stride, frame_stride, dither, h_packet_origin))
        return rc;
    if (num_packets == 0) return 0;
    if (!h_stream || !h_packet_bytes) return fail(ctx, ALAC_HIP_ParamError, "null buffer");
    if (num_packets > 0x7fffffffu) return fail(ctx, ALAC_HIP_ParamError, "more packets than the return value counts");
    uint64_t span = 0;
    if (!host_span(&c.fmt, h_num_samples_expected, num_packets, channel_stride, frame_stride, sizeof(float), span))
        return fail(ctx, ALAC_HIP_ParamError, "the largest index into h_in overflows 64 bits");
    // nothing expected anywhere: one float the kernels never load keeps the staged source a buffer
    static const float kNone = 0.0f;
    verify_float_mode(c, channel_stride, frame_stride, dither, nullptr);  // (the origins: staged by decode_host_common)
    HostDecode h{h_stream, h_packet_bytes, num_packets, (span ? span : 1) * sizeof(float)};
    h.expected = span ? h_in : &kNone, h.numSamplesExpected = h_num_samples_expected;
    h.origin = dither_on(dither) ? h_packet_origin : nullptr;
    h.firstMismatch = h_first_mismatch, h.status = h_status;
    return decode_host_common(ctx, c, h);
}

}  // extern "C"
