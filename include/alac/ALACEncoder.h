/*
 * ALACEncoder.h — drop-in for the reference's class ALACEncoder (codec/ALACEncoder.h:34-102): same method
 * names, argument meaning and int32 status codes, backed by the HIP path (libalac_hip.so).  The fork's
 * extra `index` / `X` arguments are accepted; the upstream (Apple) signatures are the same calls with the
 * defaults.  No device pointers are exposed (the fork's six public d_/dev_ members are gone).
 */
#ifndef ALAC_AMD_ENCODER_H
#define ALAC_AMD_ENCODER_H

#include <stdint.h>
#include <vector>

#include "ALACAudioTypes.h"

struct alac_hip_ctx;
struct alac_hip_float_report;
struct alac_hip_int_report;
struct alac_hip_int_source;

class ALACEncoder {
public:
    ALACEncoder();
    virtual ~ALACEncoder();

    /* codec/ALACEncoder.h:40-41.  *ioNumBytes in = PCM bytes of this packet, out = packet bytes.
     * After InitializeSampling(..., X, ...) packet `index` was already encoded in the batch and is just
     * copied out; otherwise the packet is encoded now (chained to the previous call's state). */
    virtual int32_t Encode(AudioFormatDescription theInputFormat, AudioFormatDescription theOutputFormat,
                           unsigned char *theReadBuffer, unsigned char *theWriteBuffer, int32_t *ioNumBytes,
                           int index = -1);
    virtual int32_t Finish();

    void SetFastMode(bool fast) { mFastMode = fast; }
    // Extension: independent packets with per-packet LPC coefficients (option "lpc" of include/alac_hip.h); together
    // with SetFastMode(true) every encode call fails with kALAC_ParamError.  Mono and stereo only.
    void SetLPCMode(bool lpc) { mLPCMode = lpc; }
    void SetFrameSize(uint32_t frameSize) { mFrameSize = frameSize; } /* before InitializeEncoder */
    /* Extension: the HIP device this object's context is created on (before InitializeEncoder; default: environment
     * ALAC_HIP_DEVICE, else 0).  One object = one device = one stream; objects on different devices may be driven from
     * different threads (alacconvert --batch --devices N). */
    void SetDevice(int device) { mDevice = device; }
    /* Extension: TPDF dither for the float encode methods (alac_hip_encode_float_dither; mode ALAC_HIP_DITHER_NONE = 0 or
     * ALAC_HIP_DITHER_TPDF = 1, 16 / 20 / 24 bits).  Default: none.  The integer encode methods never dither,
     * except EncodeSegmentsInt where it reduces the bit depth. */
    void SetDither(uint32_t mode, uint64_t seed) { mDitherMode = mode, mDitherSeed = seed; }

    void GetConfig(ALACSpecificConfig &config);
    uint32_t GetMagicCookieSize(uint32_t inNumChannels);
    void GetMagicCookie(void *config, uint32_t *ioSize);
    virtual int32_t InitializeEncoder(AudioFormatDescription theOutputFormat, int X = 0);

    /* codec/ALACEncoder.h:53 / ALACEncoder.cu:1385: d_ip = DEVICE buffer holding X packets at a stride of
     * outBytes[0] bytes, outBytes[i] = PCM bytes of packet i.  The whole chained encode of the X packets
     * runs here on the GPU; Encode(index) then returns packet `index`. */
    void InitializeSampling(void *d_ip, AudioFormatDescription theInputFormat, int X, int32_t *outBytes);

    /* Batch extension (host buffers): totalSamples sample-frames of packed LE PCM; segmentPackets = 0
     * chains everything to this object's state, k > 0 restarts from init_coefs every k packets. */
    int32_t EncodeBatch(const void *pcm, uint64_t totalSamples, uint32_t segmentPackets, uint8_t *out,
                        uint64_t outCapacity, uint32_t *packetBytes, uint64_t *outTotalBytes);

    /* Multi-stream form: packets back to back at the full-packet stride (frameSize * bytesPerFrame), packet p
     * holding numSamples[p] frames; segment s = packets [segFirst[s], segFirst[s+1]) is one independent stream
     * (one input file) starting from the initial coefficient state. */
    int32_t EncodeSegments(const void *pcm, const uint32_t *numSamples, uint32_t numPackets, const uint32_t *segFirst,
                           uint32_t numSegments, uint8_t *out, uint64_t outCapacity, uint32_t *packetBytes,
                           uint64_t *outTotalBytes);
    /* EncodeSegments from float32 PCM (alac_hip_encode_float_host): sample i of channel c of packet p at
     * pcm[c * channelStride + (p * frameSize + i) * frameStride], quantized to the encoder's bit depth on the GPU by the
     * rule of alac_hip.h; clipped: [numPackets] clipped samples per packet, or NULL.  No reference counterpart. */
    int32_t EncodeSegmentsFloat(const float *pcm, uint64_t channelStride, uint64_t frameStride, const uint32_t *numSamples,
                                uint32_t numPackets, const uint32_t *segFirst, uint32_t numSegments, uint8_t *out,
                                uint64_t outCapacity, uint32_t *packetBytes, uint64_t *outTotalBytes, uint32_t *clipped);
    /* EncodeSegmentsFloat with every packet's first stream frame index, packetOrigin[numPackets] (NULL: packet p starts at
     * p * frameSize): the dither set by SetDither is keyed on it, so a file whose packets count from 0 gets the same bytes
     * alone and inside a batch.  Without dither the table is ignored and the result is EncodeSegmentsFloat's. */
    int32_t EncodeSegmentsFloatAt(const float *pcm, uint64_t channelStride, uint64_t frameStride, const uint32_t *numSamples,
                                  uint32_t numPackets, const uint32_t *segFirst, uint32_t numSegments, uint8_t *out,
                                  uint64_t outCapacity, uint32_t *packetBytes, uint64_t *outTotalBytes, uint32_t *clipped,
                                  const uint64_t *packetOrigin);

    /* EncodeSegments from integer PCM of any layout, container and depth (alac_hip_encode_int_host): src describes the
     * containers of pcm, their significant bits and their strides; widened exactly or reduced to the encoder's bit depth on
     * the GPU by the integer rule of alac_hip.h.  The dither set by SetDither applies where the depth is reduced (a call that
     * widens or keeps the depth with dither set is refused, as by alac_hip_encode_int); packetOrigin as in
     * EncodeSegmentsFloatAt, or NULL.  clipped: [numPackets] clipped samples per packet, or NULL.  No reference counterpart. */
    int32_t EncodeSegmentsInt(const void *pcm, const alac_hip_int_source &src, const uint32_t *numSamples, uint32_t numPackets,
                              const uint32_t *segFirst, uint32_t numSegments, uint8_t *out, uint64_t outCapacity,
                              uint32_t *packetBytes, uint64_t *outTotalBytes, uint32_t *clipped, const uint64_t *packetOrigin);

    /* Extension: what names the lossless bit depth of float32 PCM (alac_hip_float_probe_host): the sample of channel c and
     * frame t at pcm[c * channelStride + t * frameStride]; segment s = frames [segFirstFrame[s], segFirstFrame[s + 1]) (NULL
     * with numSegments 1: all totalFrames) gets reports[s], which alac_hip_float_report_depth turns into 16, 20, 24, 32 or 0.
     * Needs no InitializeEncoder: the channel count is the call's, and the object's context is created where it is missing. */
    int32_t ProbeFloat(const float *pcm, uint32_t numChannels, uint64_t channelStride, uint64_t frameStride,
                       uint64_t totalFrames, const uint64_t *segFirstFrame, uint32_t numSegments,
                       alac_hip_float_report *reports);

    /* Extension: what names the lossless bit depth of integer PCM (alac_hip_int_probe_host): src describes the containers of
     * pcm as for EncodeSegmentsInt, the container of channel c and frame t at index c * src.channel_stride + t *
     * src.frame_stride; segments and reports as in ProbeFloat, the reports read by alac_hip_int_report_depth.  Needs no
     * InitializeEncoder. */
    int32_t ProbeInt(const void *pcm, const alac_hip_int_source &src, uint32_t numChannels, uint64_t totalFrames,
                     const uint64_t *segFirstFrame, uint32_t numSegments, alac_hip_int_report *reports);
    /* Extension: the conversion of EncodeSegmentsInt alone (alac_hip_pcm_requantize_host): numPackets packets of frameSize
     * frames of the source, packet p holding numSamples[p] of them (NULL: all full), into packed interleaved PCM of bitDepth
     * bits in out (numPackets full packets; frames behind numSamples[p] are zero).  dither: ALAC_HIP_DITHER_TPDF where the depth
     * is reduced; the packets' frames count from 0.  clipped: [numPackets] clipped samples per packet, or NULL.  Needs no
     * InitializeEncoder: the format is the call's. */
    int32_t RequantizeInt(const void *pcm, const alac_hip_int_source &src, uint32_t numChannels, uint32_t bitDepth,
                          uint32_t frameSize, const uint32_t *numSamples, uint32_t numPackets, uint8_t *out,
                          uint64_t outCapacity, uint32_t *clipped, uint32_t ditherMode, uint64_t ditherSeed);

    int32_t LastStatus() const { return mLastStatus; }

protected:
    int16_t mBitDepth;
    bool mFastMode;
    bool mLPCMode = false;
    uint32_t mDitherMode = 0;
    uint64_t mDitherSeed = 0;
    uint32_t mTotalBytesGenerated, mAvgBitRate, mMaxFrameBytes;
    uint32_t mFrameSize, mMaxOutputBytes, mNumChannels, mOutputSampleRate;

private:
    alac_hip_ctx *mCtx;
    int mDevice; /* -1: ALAC_HIP_DEVICE or 0 */
    int16_t mState[64 * 8]; /* rows 3 and 7 of mCoefsU/V[first channel of every element] (codec/ALACEncoder.h:89-90) */
    bool mStateValid;
    std::vector<uint8_t> mBatchStream;
    std::vector<uint32_t> mBatchSizes;
    std::vector<uint64_t> mBatchOffsets;
    int32_t mLastStatus;
    void account(uint32_t outputSize);
    int32_t ensureContext();
};

#endif
