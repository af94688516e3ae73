// ALACEncoder.cpp — host C++ mirror of the reference's ALACEncoder (codec/ALACEncoder.cu) over the
// alac_hip C-ABI.  Control flow that lived in EncodeStereo/EncodeMono now lives in the HIP kernels;
// this class only keeps the reference's object model (stateful encoder, cookie, statistics).
#include "alac/ALACEncoder.h"
#include "alac_hip.h"

#include "alac_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

namespace {
inline uint32_t bps_of(int depth) { return depth == 16 ? 2u : (depth == 32 ? 4u : 3u); }
inline uint32_t be32(uint32_t v) { return __builtin_bswap32(v); }
inline uint16_t be16(uint16_t v) { return (uint16_t)((v << 8) | (v >> 8)); }

// SetFastMode (EncodeStereoFast, codec/ALACEncoder.cu:998-1001) and SetLPCMode onto the context, and the calls' format
int32_t prepare(alac_hip_ctx *ctx, bool fast, bool lpc, uint32_t frameSize, int16_t bitDepth, uint32_t channels, uint32_t rate,
                alac_hip_format &fmt)
{
    fmt = {frameSize, (uint32_t)bitDepth, channels, rate};
    const int32_t rc = alac_hip_set_option(ctx, "fast_mode", fast ? 1 : 0);
    return rc != ALAC_HIP_noErr ? rc : alac_hip_set_option(ctx, "lpc", lpc ? 1 : 0);
}
}  // namespace

ALACEncoder::ALACEncoder()
    : mBitDepth(0), mFastMode(false), mTotalBytesGenerated(0), mAvgBitRate(0), mMaxFrameBytes(0),
      mFrameSize(kALACDefaultFrameSize), mMaxOutputBytes(0), mNumChannels(0), mOutputSampleRate(0), mCtx(nullptr),
      mDevice(-1), mStateValid(false), mLastStatus(0)
{
    memset(mState, 0, sizeof(mState));
}

ALACEncoder::~ALACEncoder()
{
    if (mCtx) alac_hip_destroy(mCtx);
}

// the object's context, on SetDevice's device (else ALAC_HIP_DEVICE, else 0)
int32_t ALACEncoder::ensureContext()
{
    if (mCtx) return ALAC_noErr;
    const char *dev = getenv("ALAC_HIP_DEVICE");
    const int32_t rc = alac_hip_create(&mCtx, mDevice >= 0 ? mDevice : (dev ? atoi(dev) : 0), nullptr);
    return rc != ALAC_HIP_noErr ? kALAC_MemFullError : ALAC_noErr;
}

int32_t ALACEncoder::ProbeFloat(const float *pcm, uint32_t numChannels, uint64_t channelStride, uint64_t frameStride,
                                uint64_t totalFrames, const uint64_t *segFirstFrame, uint32_t numSegments,
                                alac_hip_float_report *reports)
{
    if ((mLastStatus = ensureContext())) return mLastStatus;
    mLastStatus = alac_hip_float_probe_host(mCtx, pcm, numChannels, channelStride, frameStride, totalFrames, segFirstFrame,
                                            numSegments, reports);
    return mLastStatus;
}

int32_t ALACEncoder::ProbeInt(const void *pcm, const alac_hip_int_source &src, uint32_t numChannels, uint64_t totalFrames,
                              const uint64_t *segFirstFrame, uint32_t numSegments, alac_hip_int_report *reports)
{
    if ((mLastStatus = ensureContext())) return mLastStatus;
    mLastStatus = alac_hip_int_probe_host(mCtx, pcm, &src, numChannels, totalFrames, segFirstFrame, numSegments, reports);
    return mLastStatus;
}

int32_t ALACEncoder::RequantizeInt(const void *pcm, const alac_hip_int_source &src, uint32_t numChannels, uint32_t bitDepth,
                                   uint32_t frameSize, const uint32_t *numSamples, uint32_t numPackets, uint8_t *out,
                                   uint64_t outCapacity, uint32_t *clipped, uint32_t ditherMode, uint64_t ditherSeed)
{
    if ((mLastStatus = ensureContext())) return mLastStatus;
    const alac_hip_format fmt = {frameSize, bitDepth, numChannels, 44100};  // (the sample rate plays no part in the conversion)
    const alac_hip_dither dither = {ditherMode, 0, ditherSeed};
    mLastStatus = alac_hip_pcm_requantize_host(mCtx, &fmt, pcm, &src, numSamples, numPackets, out, outCapacity, clipped, &dither,
                                               nullptr);
    return mLastStatus;
}

// codec/ALACEncoder.cu:1457-1535
int32_t ALACEncoder::InitializeEncoder(AudioFormatDescription theOutputFormat, int /*X*/)
{
    mOutputSampleRate = (uint32_t)theOutputFormat.mSampleRate;
    mNumChannels = theOutputFormat.mChannelsPerFrame;
    switch (theOutputFormat.mFormatFlags) {
    case 1: mBitDepth = 16; break;
    case 2: mBitDepth = 20; break;
    case 3: mBitDepth = 24; break;
    case 4: mBitDepth = 32; break;
    default: break;
    }
    if (!(mBitDepth == 16 || mBitDepth == 20 || mBitDepth == 24 || mBitDepth == 32)) return kALAC_ParamError;
    if (mNumChannels < 1 || mNumChannels > kALACMaxChannels) return kALAC_ParamError;
    mMaxOutputBytes = mFrameSize * mNumChannels * ((10 + 32) / 8) + 1;        // :1489
    if (int32_t rc = ensureContext()) return rc;
    mStateValid = false;  // every row = init_coefs (:1524-1531)
    mBatchStream.clear();
    mBatchSizes.clear();
    mBatchOffsets.clear();
    return ALAC_noErr;
}

// codec/ALACEncoder.cu:1082-1095 (fields big-endian in the struct)
void ALACEncoder::GetConfig(ALACSpecificConfig &config)
{
    config.frameLength = be32(mFrameSize);
    config.compatibleVersion = (uint8_t)kALACCompatibleVersion;
    config.bitDepth = (uint8_t)mBitDepth;
    config.pb = 40;
    config.kb = 14;
    config.mb = 10;
    config.numChannels = (uint8_t)mNumChannels;
    config.maxRun = be16(255);
    config.maxFrameBytes = be32(mMaxFrameBytes);
    config.avgBitRate = be32(mAvgBitRate);
    config.sampleRate = be32(mOutputSampleRate);
}

// :1097-1107
uint32_t ALACEncoder::GetMagicCookieSize(uint32_t inNumChannels)
{
    return inNumChannels > 2 ? (uint32_t)sizeof(ALACSpecificConfig) + 24u : (uint32_t)sizeof(ALACSpecificConfig);
}

// :1109-1140
void ALACEncoder::GetMagicCookie(void *outCookie, uint32_t *ioSize)
{
    ALACSpecificConfig cfg;
    GetConfig(cfg);
    const uint32_t need = GetMagicCookieSize(mNumChannels);
    if (*ioSize >= need) {
        memcpy(outCookie, &cfg, sizeof(cfg));
        if (need > sizeof(cfg)) {  // 'chan' atom + ALACAudioChannelLayout (:1118-1133)
            uint8_t full[48];
            alac_hip_format fmt = {mFrameSize, (uint32_t)mBitDepth, mNumChannels, mOutputSampleRate};
            alac_hip_magic_cookie_full(&fmt, mMaxFrameBytes, mAvgBitRate, full, sizeof(full));
            memcpy((uint8_t *)outCookie + sizeof(cfg), full + 24, 24);
        }
        *ioSize = need;
    } else {
        *ioSize = 0;  // no incomplete cookies
    }
}

void ALACEncoder::account(uint32_t outputSize)
{
    mTotalBytesGenerated += outputSize;  // :1050-1051
    if (outputSize > mMaxFrameBytes) mMaxFrameBytes = outputSize;
}

int32_t ALACEncoder::EncodeBatch(const void *pcm, uint64_t totalSamples, uint32_t segmentPackets, uint8_t *out,
                                 uint64_t outCapacity, uint32_t *packetBytes, uint64_t *outTotalBytes)
{
    alac_hip_format fmt;  // (a null context: kALAC_ParamError from the first option call)
    if ((mLastStatus = prepare(mCtx, mFastMode, mLPCMode, mFrameSize, mBitDepth, mNumChannels, mOutputSampleRate, fmt)))
        return mLastStatus;
    const uint64_t np = (totalSamples + mFrameSize - 1) / mFrameSize;
    const uint64_t nseg = segmentPackets ? (np + segmentPackets - 1) / segmentPackets : 1;
    const uint32_t stateInt16 = alac_hip_state_int16(&fmt);  // 64 per element of a packet
    std::vector<int16_t> state(nseg * stateInt16, 0);
    const bool chain = (segmentPackets == 0) && mStateValid;
    if (chain) memcpy(state.data(), mState, stateInt16 * 2u);
    uint64_t total = 0;
    mLastStatus = alac_hip_encode_host(mCtx, &fmt, pcm, totalSamples, segmentPackets, state.data(), chain ? 1 : 0, out,
                                       outCapacity, packetBytes, &total);
    if (mLastStatus != ALAC_HIP_noErr) return mLastStatus;
    if (segmentPackets == 0 && np && !mLPCMode) {  // LPC packets leave no predictor state behind
        memcpy(mState, state.data(), stateInt16 * 2u);
        mStateValid = true;
    }
    for (uint64_t p = 0; p < np; p++) account(packetBytes[p]);
    if (outTotalBytes) *outTotalBytes = total;
    return ALAC_noErr;
}

int32_t ALACEncoder::EncodeSegments(const void *pcm, const uint32_t *numSamples, uint32_t numPackets,
                                    const uint32_t *segFirst, uint32_t numSegments, uint8_t *out, uint64_t outCapacity,
                                    uint32_t *packetBytes, uint64_t *outTotalBytes)
{
    alac_hip_format fmt;  // (a null context: kALAC_ParamError from the first option call)
    if ((mLastStatus = prepare(mCtx, mFastMode, mLPCMode, mFrameSize, mBitDepth, mNumChannels, mOutputSampleRate, fmt)))
        return mLastStatus;
    uint64_t total = 0;
    mLastStatus = alac_hip_encode_host_segments(mCtx, &fmt, pcm, numSamples, numPackets, segFirst, numSegments, nullptr, 0,
                                                out, outCapacity, packetBytes, &total);
    if (mLastStatus != ALAC_HIP_noErr) return mLastStatus;
    for (uint32_t p = 0; p < numPackets; p++) account(packetBytes[p]);
    if (outTotalBytes) *outTotalBytes = total;
    return ALAC_noErr;
}

int32_t ALACEncoder::EncodeSegmentsFloat(const float *pcm, uint64_t channelStride, uint64_t frameStride,
                                         const uint32_t *numSamples, uint32_t numPackets, const uint32_t *segFirst,
                                         uint32_t numSegments, uint8_t *out, uint64_t outCapacity, uint32_t *packetBytes,
                                         uint64_t *outTotalBytes, uint32_t *clipped)
{
    return EncodeSegmentsFloatAt(pcm, channelStride, frameStride, numSamples, numPackets, segFirst, numSegments, out,
                                 outCapacity, packetBytes, outTotalBytes, clipped, nullptr);
}

int32_t ALACEncoder::EncodeSegmentsFloatAt(const float *pcm, uint64_t channelStride, uint64_t frameStride,
                                           const uint32_t *numSamples, uint32_t numPackets, const uint32_t *segFirst,
                                           uint32_t numSegments, uint8_t *out, uint64_t outCapacity, uint32_t *packetBytes,
                                           uint64_t *outTotalBytes, uint32_t *clipped, const uint64_t *packetOrigin)
{
    alac_hip_format fmt;  // (a null context: kALAC_ParamError from the first option call)
    if ((mLastStatus = prepare(mCtx, mFastMode, mLPCMode, mFrameSize, mBitDepth, mNumChannels, mOutputSampleRate, fmt)))
        return mLastStatus;
    uint64_t total = 0;
    const alac_hip_dither dither = {mDitherMode, 0, mDitherSeed};
    mLastStatus = alac_hip_encode_float_dither_host(mCtx, &fmt, pcm, channelStride, frameStride, numSamples, numPackets,
                                                    segFirst, numSegments, nullptr, 0, out, outCapacity, packetBytes, &total,
                                                    clipped, &dither, packetOrigin);
    if (mLastStatus != ALAC_HIP_noErr) return mLastStatus;
    for (uint32_t p = 0; p < numPackets; p++) account(packetBytes[p]);
    if (outTotalBytes) *outTotalBytes = total;
    return ALAC_noErr;
}

int32_t ALACEncoder::EncodeSegmentsInt(const void *pcm, const alac_hip_int_source &src, const uint32_t *numSamples,
                                       uint32_t numPackets, const uint32_t *segFirst, uint32_t numSegments, uint8_t *out,
                                       uint64_t outCapacity, uint32_t *packetBytes, uint64_t *outTotalBytes, uint32_t *clipped,
                                       const uint64_t *packetOrigin)
{
    alac_hip_format fmt;  // (a null context: kALAC_ParamError from the first option call)
    if ((mLastStatus = prepare(mCtx, mFastMode, mLPCMode, mFrameSize, mBitDepth, mNumChannels, mOutputSampleRate, fmt)))
        return mLastStatus;
    uint64_t total = 0;
    const alac_hip_dither dither = {mDitherMode, 0, mDitherSeed};
    mLastStatus = alac_hip_encode_int_host(mCtx, &fmt, pcm, &src, numSamples, numPackets, segFirst, numSegments, nullptr, 0, out,
                                           outCapacity, packetBytes, &total, clipped, &dither, packetOrigin);
    if (mLastStatus != ALAC_HIP_noErr) return mLastStatus;
    for (uint32_t p = 0; p < numPackets; p++) account(packetBytes[p]);
    if (outTotalBytes) *outTotalBytes = total;
    return ALAC_noErr;
}

// codec/ALACEncoder.cu:1385-1451
void ALACEncoder::InitializeSampling(void *d_ip, AudioFormatDescription theInputFormat, int X, int32_t *outBytes)
{
    mLastStatus = kALAC_ParamError;
    if (!mCtx || X <= 0 || !d_ip || !outBytes) return;
    const uint32_t bpf = theInputFormat.mChannelsPerFrame * bps_of(mBitDepth);
    const int64_t stride = outBytes[0];
    if (stride != (int64_t)mFrameSize * bpf) return;  // first packet must be full, as the fork assumes (:1153)
    // packets the caller really filled: main.cu leaves the tail entries of outBytes[] unset when the file
    // is an exact multiple (X = bytes/packet + 1, convert-utility/main.cu:409) — drop anything implausible
    std::vector<uint32_t> ns;
    for (int i = 0; i < X; i++) {
        const int64_t b = outBytes[i];
        if (b <= 0 || b > stride || (b % bpf) != 0) break;
        ns.push_back((uint32_t)(b / bpf));
        if (b != stride) break;  // a partial packet ends the stream
    }
    const uint32_t np = (uint32_t)ns.size();
    if (np == 0) return;
    alac_hip_format fmt;
    if ((mLastStatus = prepare(mCtx, mFastMode, mLPCMode, mFrameSize, mBitDepth, mNumChannels, mOutputSampleRate, fmt))) return;
    const uint32_t segFirst[2] = {0, np};
    const uint64_t wsBytes = alac_hip_encode_workspace_bytes(&fmt, np, mLPCMode ? np : 1);
    const uint64_t outMax = alac_hip_encode_max_output_bytes(&fmt, np);
    std::unique_ptr<uint8_t[]> out(new uint8_t[outMax]);  // (not value-initialised: only the stream's bytes are written)
    mBatchSizes.assign(np, 0);
    uint64_t total = 0;
    // one chained segment of np packets from the caller's device buffer: its bound is known, so the library does not read
    // the table back.  alac_hip_synchronize reads the context's hand-off error word: a consumer wave that gave up waiting for
    // its producer has coded garbage, and the batch must fail instead of being handed out.
    mLastStatus = alachost::encode_host_common(
        (hipStream_t)alac_hip_stream(mCtx), &fmt,
        {ns.data(), np, segFirst, 1, mState, mStateValid ? 1 : 0, out.get(), outMax, mBatchSizes.data(), &total}, wsBytes,
        [&](const alachost::StagedEncode &d) {
            return alac_hip_encode_segmented(mCtx, &fmt, d_ip, d.numSamples, np, d.segFirst, 1, d.maxSeg, d.state, d.stateIn, d.ws,
                                             wsBytes, d.out, d.outCapacity, d.packetBytes, d.offsets);
        },
        [](int32_t code, const char *, hipError_t) { return code; }, [&] { return alac_hip_synchronize(mCtx); });
    const bool ok = mLastStatus == ALAC_HIP_noErr;  // (a failed batch hands out nothing)
    mBatchStream.assign(out.get(), out.get() + (ok ? total : 0));
    mBatchSizes.resize(ok ? np : 0);
    mBatchOffsets.assign(ok ? np + 1 : 0, 0);
    for (uint32_t p = 0; p < mBatchSizes.size(); p++) mBatchOffsets[p + 1] = mBatchOffsets[p] + mBatchSizes[p];
    mStateValid = mStateValid || ok;
}

// codec/ALACEncoder.cu:973-1057
int32_t ALACEncoder::Encode(AudioFormatDescription theInputFormat, AudioFormatDescription /*theOutputFormat*/,
                            unsigned char *theReadBuffer, unsigned char *theWriteBuffer, int32_t *ioNumBytes,
                            int index)
{
    if (!mCtx || !ioNumBytes || !theWriteBuffer) return kALAC_ParamError;
    if (theInputFormat.mChannelsPerFrame != mNumChannels) return kALAC_ParamError;
    // batch already encoded by InitializeSampling: hand out packet `index`
    if (index >= 0 && (size_t)index < mBatchSizes.size()) {
        const uint32_t n = mBatchSizes[index];
        memcpy(theWriteBuffer, mBatchStream.data() + mBatchOffsets[index], n);
        *ioNumBytes = (int32_t)n;
        account(n);
        return ALAC_noErr;
    }
    if (!theReadBuffer) return kALAC_ParamError;
    const uint32_t bpf = mNumChannels * bps_of(mBitDepth);
    const uint32_t numFrames = (uint32_t)*ioNumBytes / (theInputFormat.mBytesPerPacket ? theInputFormat.mBytesPerPacket : bpf);
    if (numFrames > mFrameSize) return kALAC_ParamError;
    uint32_t nb = 0;
    uint64_t total = 0;
    std::vector<uint8_t> tmp((size_t)mFrameSize * bpf + 64);
    int32_t rc = EncodeBatch(theReadBuffer, numFrames, 0, tmp.data(), tmp.size(), &nb, &total);
    if (rc != ALAC_noErr) return rc;
    memcpy(theWriteBuffer, tmp.data(), total);
    *ioNumBytes = (int32_t)total;
    return ALAC_noErr;
}

// :1064-1073 (a no-op in the reference)
int32_t ALACEncoder::Finish() { return ALAC_noErr; }
