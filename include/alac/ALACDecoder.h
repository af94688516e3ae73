/*
 * ALACDecoder.h — drop-in for the reference's class ALACDecoder (codec/ALACDecoder.h:38-72), backed by
 * the HIP path.  Both the upstream (Apple) Decode signature (host sampleBuffer) and the fork's
 * (Decode(..., X) + fillWriteBuffer into a device buffer) are provided.
 */
#ifndef ALAC_AMD_DECODER_H
#define ALAC_AMD_DECODER_H

#include <stdint.h>
#include <vector>

#include "ALACAudioTypes.h"

struct alac_hip_ctx;
struct alac_hip_pcm_digest;
struct alac_hip_int_source;

class ALACDecoder {
public:
    ALACDecoder();
    ~ALACDecoder();

    /* codec/ALACDecoder.cu:109-190 */
    int32_t Init(void *inMagicCookie, uint32_t inMagicCookieSize, int X = 0);
    /* Extension: the HIP device of this object's context (before Init; default: environment ALAC_HIP_DEVICE, else 0) */
    void SetDevice(int device) { mDevice = device; }

    /* upstream form: decode the packet at bits->cur into host sampleBuffer (packed LE interleaved) */
    int32_t Decode(BitBuffer *bits, uint8_t *sampleBuffer, uint32_t numSamples, uint32_t numChannels,
                   uint32_t *outNumSamples);

    /* fork form (codec/ALACDecoder.h:45-46): queue packet X (bytes bits->cur .. bits->end), report its
     * sample count; fillWriteBuffer decodes every queued packet on the GPU straight into the DEVICE
     * buffer, packet X at X * theOutputPacketBytes. */
    int32_t Decode(BitBuffer *bits, uint32_t numSamples, uint32_t numChannels, uint32_t *outNumSamples,
                   uint32_t outBytesPerPacket, int X);
    void fillWriteBuffer(void *deviceSampleBuffer, uint32_t numChannels, int32_t theOutputPacketBytes, int X);

    /* batch extension (host buffers) */
    int32_t DecodeBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets, uint8_t *pcmOut,
                        uint32_t *numSamplesOut, int32_t *statusOut);
    /* batch extension (host buffers): DecodeBatch into integer containers of the caller's layout (alac_hip_decode_int_host).
     * dst is an alac_hip_int_source read as a destination (alac_hip_int_dest): sample i of channel c of packet p goes to the
     * container at index c * dst->channel_stride + (p * frameLength + i) * dst->frame_stride of `out`, left- or right-justified
     * by the rule of include/alac_hip.h; containers decode does not write come back as zero, the bytes between containers
     * are left alone.  numSamplesOut and statusOut as DecodeBatch. */
    int32_t DecodeBatchInt(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets, void *out,
                           const alac_hip_int_source *dst, uint32_t *numSamplesOut, int32_t *statusOut);
    /* batch extension (host buffers): decode on the device and compare with pcmExpected (the layout DecodeBatch writes)
     * without writing PCM anywhere (alac_hip_verify_host).  firstMismatchOut[p] = lowest differing sample-frame of packet p,
     * 0xFFFFFFFF if it matches; statusOut as DecodeBatch; numSamplesExpected NULL = every packet full; badPacketsOut may be
     * NULL.  Returns ALAC_noErr or a parameter / HIP error — a mismatch is not an error. */
    int32_t VerifyBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets, const uint8_t *pcmExpected,
                        const uint32_t *numSamplesExpected, uint32_t *firstMismatchOut, int32_t *statusOut,
                        uint32_t *badPacketsOut = nullptr);
    /* batch extension (host buffers): VerifyBatch against the float32 SOURCE of a float encode (alac_hip_verify_float_host).
     * Sample i of channel c of packet p is in[c * channelStride + (p * frameLength + i) * frameStride]; every decoded sample
     * is compared with what ALACEncoder::EncodeSegmentsFloat(At) stages for that float at the stream's bit depth — rounding,
     * saturation, NaN -> 0 and, with ditherMode ALAC_HIP_DITHER_TPDF, the dither of (ditherSeed, channel, packetOrigin[p] + i)
     * (packetOrigin NULL: p * frameLength).  Only frames in front of numSamplesExpected[p] are read from `in`.  Outputs and
     * return value as VerifyBatch. */
    int32_t VerifyBatchFloat(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets, const float *in,
                             uint64_t channelStride, uint64_t frameStride, const uint32_t *numSamplesExpected,
                             uint32_t ditherMode, uint64_t ditherSeed, const uint64_t *packetOrigin,
                             uint32_t *firstMismatchOut, int32_t *statusOut, uint32_t *badPacketsOut = nullptr);

    /* batch extension (host buffers): the CRC-32 of the PCM of whole files, with the PCM never leaving the device.  File j is
     * packets [fileFirstPacket[j], fileFirstPacket[j + 1]) of the batch (fileFirstPacket: numFiles + 1 entries, from 0 to
     * numPackets); the packets are decoded into a device buffer and alac_hip_pcm_crc32 runs over it with one range per file:
     * outDigests[j].crc32 is zlib's crc32 of the bytes DecodeBatch would give for the file's packets with every packet's
     * frames back to back (the `data` chunk of its WAV), outDigests[j].bytes their count.  A file with a short packet in
     * front of its last one gets one range per packet, joined with alac_hip_crc32_combine.  Only the digests, outFrames
     * [numPackets] (decoded frames per packet) and outStatus [numPackets] (as DecodeBatch) are copied back.  Returns
     * ALAC_noErr or a parameter / HIP error — an undecodable packet is reported in outStatus, not by the return value. */
    int32_t TestBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets, const uint32_t *fileFirstPacket,
                      uint32_t numFiles, alac_hip_pcm_digest *outDigests, uint32_t *outFrames, int32_t *outStatus);

    /* batch extension (host buffers): the loudness of whole files, with the PCM never leaving the device.  Files and packets as
     * in TestBatch.  The packets are decoded into a device buffer, and alac_hip_loudness_int measures one segment per file on
     * that plane — the descriptor is {the stream's bytes per sample, its depth, left-justified, channel_stride 1, frame_stride
     * numChannels}, the sample rate the cookie's — where the file's frames lie back to back (a file with a short packet in
     * front of its last one is first copied together on the device).  outLufs[j] is the integrated loudness of file j
     * (alac_hip_loudness_integrated with BS.1770's weights in the order of the stream's ALAC layout tag; -HUGE_VAL where no
     * block passes the gates), outPeak[j] its sample peak (1.0 = full scale).  Only the rows, the reports, outFrames
     * [numPackets] and outStatus [numPackets] (as TestBatch) are copied back.  Returns ALAC_noErr or a parameter / HIP error (a
     * cookie whose sample rate alac_hip_loudness_int refuses is one) — an undecodable packet is reported in outStatus, and
     * its file is not measured: -HUGE_VAL and peak 0, as for a file without frames (a batch without packets gives that for
     * every file). */
    int32_t LoudnessBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets, const uint32_t *fileFirstPacket,
                          uint32_t numFiles, double *outLufs, double *outPeak, uint32_t *outFrames, int32_t *outStatus);

    /* LoudnessBatch with both measurements taken on the one decoded plane: outTruePeak[j] is the true peak of file j (ITU-R
     * BS.1770-4 annex 2, alac_hip_true_peak_int over the same segments; 1.0 = full scale), the maximum over its channels.  The
     * other outputs and the return value are LoudnessBatch's.  A file that is not measured gives true peak 0. */
    int32_t LoudnessTruePeakBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets,
                                  const uint32_t *fileFirstPacket, uint32_t numFiles, double *outLufs, double *outPeak,
                                  double *outTruePeak, uint32_t *outFrames, int32_t *outStatus);

    int32_t LastStatus() const { return mLastStatus; }

public:
    ALACSpecificConfig mConfig;  /* host-endian copy, as in the reference (codec/ALACDecoder.cu:139-151) */

private:
    /* LoudnessBatch (outTruePeak NULL) and LoudnessTruePeakBatch */
    int32_t MeasureBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets, const uint32_t *fileFirstPacket,
                         uint32_t numFiles, double *outLufs, double *outPeak, double *outTruePeak, uint32_t *outFrames,
                         int32_t *outStatus);

    alac_hip_ctx *mCtx;
    int mDevice; /* -1: ALAC_HIP_DEVICE or 0 */
    std::vector<uint8_t> mCookie;
    std::vector<uint8_t> mQueued;         /* fork form: queued packet bytes */
    std::vector<uint32_t> mQueuedSizes;
    int32_t mLastStatus;
};

#endif
