// ALACDecoder.cpp — host C++ mirror of the reference's ALACDecoder (codec/ALACDecoder.cu) over the
// alac_hip C-ABI.
#include "alac/ALACDecoder.h"
#include "alac_hip.h"

#include "alac_host.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace {
inline uint32_t bps_of(uint32_t depth) { return depth == 16 ? 2u : (depth == 32 ? 4u : 3u); }

// sample count of the first audio element of a packet (header peek, codec/ALACDecoder.cu:621-654)
uint32_t peek_num_samples(const uint8_t *p, size_t n, uint32_t frameLength)
{
    if (n < 3) return 0;
    const uint32_t tag = p[0] >> 5;
    if (!(tag == 0 || tag == 1 || tag == 3)) return frameLength;
    // bits: 3 tag, 4 instance, 12 unused, 4 flags -> the partial flag is bit 19
    const uint32_t flags = ((p[2] >> 1) & 0xf);
    if (!(flags & 8)) return frameLength;
    if (n < 7) return 0;
    uint64_t v = 0;
    for (int i = 2; i < 7; i++) v = (v << 8) | p[i];
    return (uint32_t)((v >> 1) & 0xffffffffu);  // 32 bits starting at bit 23
}
}  // namespace

ALACDecoder::ALACDecoder() : mCtx(nullptr), mDevice(-1), mLastStatus(0) { memset(&mConfig, 0, sizeof(mConfig)); }

ALACDecoder::~ALACDecoder()
{
    if (mCtx) alac_hip_destroy(mCtx);
}

int32_t ALACDecoder::Init(void *inMagicCookie, uint32_t inMagicCookieSize, int /*X*/)
{
    alac_hip_format fmt;
    if (!inMagicCookie) return kALAC_ParamError;
    int32_t rc = alac_hip_format_from_cookie((const uint8_t *)inMagicCookie, inMagicCookieSize, &fmt);
    if (rc != ALAC_HIP_noErr) return kALAC_ParamError;
    const uint8_t *ck = (const uint8_t *)inMagicCookie;
    uint32_t size = inMagicCookieSize;
    if (size >= 12 && ck[4] == 'f' && ck[5] == 'r' && ck[6] == 'm' && ck[7] == 'a') { ck += 12; size -= 12; }
    if (size >= 12 && ck[4] == 'a' && ck[5] == 'l' && ck[6] == 'a' && ck[7] == 'c') { ck += 12; size -= 12; }
    mCookie.assign(ck, ck + 24);
    mConfig.frameLength = fmt.frame_size;
    mConfig.compatibleVersion = ck[4];
    mConfig.bitDepth = ck[5];
    mConfig.pb = ck[6];
    mConfig.mb = ck[7];
    mConfig.kb = ck[8];
    mConfig.numChannels = ck[9];
    mConfig.maxRun = (uint16_t)((ck[10] << 8) | ck[11]);
    mConfig.maxFrameBytes = ((uint32_t)ck[12] << 24) | ((uint32_t)ck[13] << 16) | ((uint32_t)ck[14] << 8) | ck[15];
    mConfig.avgBitRate = ((uint32_t)ck[16] << 24) | ((uint32_t)ck[17] << 16) | ((uint32_t)ck[18] << 8) | ck[19];
    mConfig.sampleRate = fmt.sample_rate;
    if (!mCtx) {
        const char *dev = getenv("ALAC_HIP_DEVICE");
        if (alac_hip_create(&mCtx, mDevice >= 0 ? mDevice : (dev ? atoi(dev) : 0), nullptr) != ALAC_HIP_noErr) return kALAC_MemFullError;
    }
    mQueued.clear();
    mQueuedSizes.clear();
    return ALAC_noErr;
}

int32_t ALACDecoder::DecodeBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets,
                                 uint8_t *pcmOut, uint32_t *numSamplesOut, int32_t *statusOut)
{
    if (!mCtx || mCookie.empty()) return kALAC_ParamError;
    mLastStatus = alac_hip_decode_host(mCtx, mCookie.data(), (uint32_t)mCookie.size(), stream, packetBytes, numPackets,
                                       pcmOut, numSamplesOut, statusOut);
    return mLastStatus;
}

int32_t ALACDecoder::DecodeBatchInt(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets, void *out,
                                    const alac_hip_int_source *dst, uint32_t *numSamplesOut, int32_t *statusOut)
{
    if (!mCtx || mCookie.empty()) return kALAC_ParamError;
    mLastStatus = alac_hip_decode_int_host(mCtx, mCookie.data(), (uint32_t)mCookie.size(), stream, packetBytes, numPackets, out,
                                           dst, numSamplesOut, statusOut);
    return mLastStatus;
}

int32_t ALACDecoder::VerifyBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets,
                                 const uint8_t *pcmExpected, const uint32_t *numSamplesExpected, uint32_t *firstMismatchOut,
                                 int32_t *statusOut, uint32_t *badPacketsOut)
{
    if (!mCtx || mCookie.empty() || !firstMismatchOut || !statusOut) return kALAC_ParamError;
    const int32_t bad = alac_hip_verify_host(mCtx, mCookie.data(), (uint32_t)mCookie.size(), stream, packetBytes, numPackets,
                                             pcmExpected, numSamplesExpected, firstMismatchOut, statusOut);
    mLastStatus = bad < 0 ? bad : ALAC_noErr;
    if (bad >= 0 && badPacketsOut) *badPacketsOut = (uint32_t)bad;
    return mLastStatus;
}

int32_t ALACDecoder::VerifyBatchFloat(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets, const float *in,
                                      uint64_t channelStride, uint64_t frameStride, const uint32_t *numSamplesExpected,
                                      uint32_t ditherMode, uint64_t ditherSeed, const uint64_t *packetOrigin,
                                      uint32_t *firstMismatchOut, int32_t *statusOut, uint32_t *badPacketsOut)
{
    if (!mCtx || mCookie.empty() || !firstMismatchOut || !statusOut) return kALAC_ParamError;
    const alac_hip_dither dither = {ditherMode, 0, ditherSeed};
    const int32_t bad = alac_hip_verify_float_host(mCtx, mCookie.data(), (uint32_t)mCookie.size(), stream, packetBytes, numPackets,
                                                   in, channelStride, frameStride, numSamplesExpected, &dither, packetOrigin,
                                                   firstMismatchOut, statusOut);
    mLastStatus = bad < 0 ? bad : ALAC_noErr;
    if (bad >= 0 && badPacketsOut) *badPacketsOut = (uint32_t)bad;
    return mLastStatus;
}

int32_t ALACDecoder::TestBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets,
                               const uint32_t *fileFirstPacket, uint32_t numFiles, alac_hip_pcm_digest *outDigests,
                               uint32_t *outFrames, int32_t *outStatus)
{
    if (!mCtx || mCookie.empty() || !fileFirstPacket || !outDigests || !outFrames || !outStatus) return kALAC_ParamError;
    if (numFiles == 0) return mLastStatus = ALAC_noErr;
    for (uint32_t j = 0; j < numFiles; j++)
        if (fileFirstPacket[j] > fileFirstPacket[j + 1]) return kALAC_ParamError;
    if (fileFirstPacket[0] != 0 || fileFirstPacket[numFiles] != numPackets || (numPackets && (!stream || !packetBytes)))
        return kALAC_ParamError;
    const uint32_t np = numPackets, frame = mConfig.frameLength, bpf = mConfig.numChannels * bps_of(mConfig.bitDepth);
    const uint64_t packetPcm = (uint64_t)frame * bpf;
    alac_hip_format fmt = {mConfig.frameLength, mConfig.bitDepth, mConfig.numChannels, mConfig.sampleRate};
    hipStream_t st = (hipStream_t)alac_hip_stream(mCtx);
    alachost::DevStream d;
    alachost::DevBuf dWs, dNs, dSt, dPcm, dTab, dDig;
    uint64_t wsBytes = 0;
    if (np) {
        // a failed staging step is kALAC_MemFullError here, whichever it is
        if (alachost::upload_stream(stream, packetBytes, np, st, d,
                                    [](int32_t, const char *, hipError_t) { return (int32_t)kALAC_MemFullError; }) ||
            dWs.alloc(wsBytes = alac_hip_decode_workspace_bytes_stream(&fmt, np, d.total)) || dNs.alloc(np * 4ull) ||
            dSt.alloc(np * 4ull) || dPcm.alloc(np * packetPcm))
            return mLastStatus = kALAC_MemFullError;
        mLastStatus = alac_hip_decode(mCtx, mCookie.data(), (uint32_t)mCookie.size(), (const uint8_t *)d.bytes.p,
                                      (const uint64_t *)d.offs.p, np, dWs.p, wsBytes, (uint8_t *)dPcm.p, (uint32_t *)dNs.p,
                                      (int32_t *)dSt.p);
        if (mLastStatus != ALAC_HIP_noErr) return mLastStatus;
        // the frame counts come back before the table is built: a file's frames sit back to back only when all its packets
        // but the last are full
        if (hipMemcpyAsync(outFrames, dNs.p, np * 4ull, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(outStatus, dSt.p, np * 4ull, hipMemcpyDeviceToHost, st) != hipSuccess)
            return mLastStatus = kALAC_ParamError;
        if ((mLastStatus = alac_hip_synchronize(mCtx)) != ALAC_HIP_noErr) return mLastStatus;
    }
    // one range per file; a file with a short packet in front of its last one: one range per packet, joined below
    std::vector<uint64_t> table;
    std::vector<uint32_t> firstRange(numFiles + 1, 0);
    for (uint32_t j = 0; j < numFiles; j++) {
        const uint32_t p0 = fileFirstPacket[j], p1 = fileFirstPacket[j + 1];
        bool packed = true;
        uint64_t frames = 0;
        for (uint32_t p = p0; p < p1; p++) {
            if (outFrames[p] > frame) return mLastStatus = kALAC_ParamError;  // (the decoder never reports more)
            packed = packed && (p + 1 == p1 || outFrames[p] == frame);
            frames += outFrames[p];
        }
        if (packed) {
            table.push_back(p0 * packetPcm), table.push_back(frames * bpf);
        } else {
            for (uint32_t p = p0; p < p1; p++) table.push_back(p * packetPcm), table.push_back((uint64_t)outFrames[p] * bpf);
        }
        firstRange[j + 1] = (uint32_t)(table.size() / 2);
    }
    const uint32_t nr = firstRange[numFiles];
    const uint64_t tabBytes = alac_hip_pcm_crc32_workspace_bytes(nr);
    std::vector<alac_hip_pcm_digest> dig(nr);
    if (dTab.alloc(tabBytes) || dDig.alloc(nr * 16ull)) return mLastStatus = kALAC_MemFullError;
    mLastStatus = alac_hip_pcm_crc32(mCtx, dPcm.p, np * packetPcm, table.data(), nr, dTab.p, tabBytes, (alac_hip_pcm_digest *)dDig.p);
    if (mLastStatus != ALAC_HIP_noErr) return mLastStatus;
    // only the digests cross the bus: the PCM stays on the device
    if (hipMemcpyAsync(dig.data(), dDig.p, nr * 16ull, hipMemcpyDeviceToHost, st) != hipSuccess)
        return mLastStatus = kALAC_ParamError;
    if ((mLastStatus = alac_hip_synchronize(mCtx)) != ALAC_HIP_noErr) return mLastStatus;
    for (uint32_t j = 0; j < numFiles; j++) {
        alac_hip_pcm_digest sum = {0, 0, 0};
        for (uint32_t r = firstRange[j]; r < firstRange[j + 1]; r++) {
            sum.crc32 = alac_hip_crc32_combine(sum.crc32, dig[r].crc32, dig[r].bytes);
            sum.bytes += dig[r].bytes;
        }
        outDigests[j] = sum;
    }
    return mLastStatus = ALAC_noErr;
}

int32_t ALACDecoder::LoudnessBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets,
                                   const uint32_t *fileFirstPacket, uint32_t numFiles, double *outLufs, double *outPeak,
                                   uint32_t *outFrames, int32_t *outStatus)
{
    return MeasureBatch(stream, packetBytes, numPackets, fileFirstPacket, numFiles, outLufs, outPeak, nullptr, outFrames, outStatus);
}

int32_t ALACDecoder::LoudnessTruePeakBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets,
                                           const uint32_t *fileFirstPacket, uint32_t numFiles, double *outLufs, double *outPeak,
                                           double *outTruePeak, uint32_t *outFrames, int32_t *outStatus)
{
    if (!outTruePeak) return kALAC_ParamError;
    return MeasureBatch(stream, packetBytes, numPackets, fileFirstPacket, numFiles, outLufs, outPeak, outTruePeak, outFrames,
                        outStatus);
}

// what LoudnessBatch and LoudnessTruePeakBatch share: the decode, the per-file segment table, the copy-together of files with a
// short middle packet, and the measurements on that one plane (outTruePeak NULL: the loudness call alone)
int32_t ALACDecoder::MeasureBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets,
                                  const uint32_t *fileFirstPacket, uint32_t numFiles, double *outLufs, double *outPeak,
                                  double *outTruePeak, uint32_t *outFrames, int32_t *outStatus)
{
    if (!mCtx || mCookie.empty() || !fileFirstPacket || !outLufs || !outPeak || (numPackets && (!outFrames || !outStatus)))
        return kALAC_ParamError;
    if (numFiles == 0) return mLastStatus = ALAC_noErr;
    for (uint32_t j = 0; j < numFiles; j++)
        if (fileFirstPacket[j] > fileFirstPacket[j + 1]) return kALAC_ParamError;
    if (fileFirstPacket[0] != 0 || fileFirstPacket[numFiles] != numPackets || (numPackets && (!stream || !packetBytes)))
        return kALAC_ParamError;
    const uint32_t np = numPackets, frame = mConfig.frameLength, C = mConfig.numChannels, bps = bps_of(mConfig.bitDepth);
    const uint64_t bpf = (uint64_t)C * bps, packetPcm = frame * bpf;
    if (np == 0) {  // files without packets: no frames, so neither a loudness nor a peak
        for (uint32_t j = 0; j < numFiles; j++) {
            outLufs[j] = -HUGE_VAL, outPeak[j] = 0.0;
            if (outTruePeak) outTruePeak[j] = 0.0;
        }
        return mLastStatus = ALAC_noErr;
    }
    alac_hip_format fmt = {mConfig.frameLength, mConfig.bitDepth, mConfig.numChannels, mConfig.sampleRate};
    hipStream_t st = (hipStream_t)alac_hip_stream(mCtx);
    alachost::DevStream d;
    alachost::DevBuf dWs, dNs, dSt, dPcm, dPacked, dLoudWs, dRows, dRep, dPeakWs, dPeaks, dPeakRep;
    uint64_t wsBytes = 0;
    if (np) {
        if (alachost::upload_stream(stream, packetBytes, np, st, d,
                                    [](int32_t, const char *, hipError_t) { return (int32_t)kALAC_MemFullError; }) ||
            dWs.alloc(wsBytes = alac_hip_decode_workspace_bytes_stream(&fmt, np, d.total)) || dNs.alloc(np * 4ull) ||
            dSt.alloc(np * 4ull) || dPcm.alloc(np * packetPcm))
            return mLastStatus = kALAC_MemFullError;
        mLastStatus = alac_hip_decode(mCtx, mCookie.data(), (uint32_t)mCookie.size(), (const uint8_t *)d.bytes.p,
                                      (const uint64_t *)d.offs.p, np, dWs.p, wsBytes, (uint8_t *)dPcm.p, (uint32_t *)dNs.p,
                                      (int32_t *)dSt.p);
        if (mLastStatus != ALAC_HIP_noErr) return mLastStatus;
        if (hipMemcpyAsync(outFrames, dNs.p, np * 4ull, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(outStatus, dSt.p, np * 4ull, hipMemcpyDeviceToHost, st) != hipSuccess)
            return mLastStatus = kALAC_ParamError;
        if ((mLastStatus = alac_hip_synchronize(mCtx)) != ALAC_HIP_noErr) return mLastStatus;
    }
    // one segment per file, in frames of the plane; a file's frames sit back to back only when all its packets but the last
    // are full.  A file with an undecodable packet is not measured (its segment is empty: -HUGE_VAL and peak 0, and outStatus
    // names the packet), so that one damaged file does not send the whole batch through the copy below.
    std::vector<uint64_t> table(numFiles + 1, 0);
    bool packed = true;
    for (uint32_t j = 0; j < numFiles; j++) {
        const uint32_t p0 = fileFirstPacket[j], p1 = fileFirstPacket[j + 1];
        uint64_t frames = 0;
        bool whole = true, filePacked = true;
        for (uint32_t p = p0; p < p1; p++) {
            if (outFrames[p] > frame) return mLastStatus = kALAC_ParamError;  // (the decoder never reports more)
            whole = whole && outStatus[p] == 0;
            filePacked = filePacked && (p + 1 == p1 || outFrames[p] == frame);
            frames += outFrames[p];
        }
        packed = packed && (!whole || filePacked);
        table[j + 1] = table[j] + (whole ? frames : 0);
    }
    const void *plane = dPcm.p;
    std::vector<uint64_t> seg(2 * (size_t)numFiles + 1, 0);  // packed: [file start, file end) per file, the slack between them
    uint32_t nseg = numFiles;                               // as segments of its own that nobody reads
    if (!packed) {
        // (a file with a short packet in front of its last one: rare; one copy per packet of the batch's measured files)
        // every packet's frames copied together into a second plane, where segment j is [table[j], table[j + 1])
        if (dPacked.alloc(table[numFiles] * bpf)) return mLastStatus = kALAC_MemFullError;
        uint64_t at = 0;
        for (uint32_t j = 0; j < numFiles; j++) {
            if (table[j + 1] == table[j]) continue;  // empty, or not measured
            for (uint32_t p = fileFirstPacket[j]; p < fileFirstPacket[j + 1]; p++) {
                if (outFrames[p] && hipMemcpyAsync((uint8_t *)dPacked.p + at * bpf, (const uint8_t *)dPcm.p + p * packetPcm,
                                                   outFrames[p] * bpf, hipMemcpyDeviceToDevice, st) != hipSuccess)
                    return mLastStatus = kALAC_ParamError;
                at += outFrames[p];
            }
        }
        plane = dPacked.p;
        seg.assign(table.begin(), table.end());
    } else {
        // file j lies at its first packet's place: segment 2j is the file, segment 2j + 1 what lies behind it up to the next
        nseg = 2 * numFiles;
        for (uint32_t j = 0; j < numFiles; j++) {
            seg[2 * j] = (uint64_t)fileFirstPacket[j] * frame;
            seg[2 * j + 1] = seg[2 * j] + (table[j + 1] - table[j]);
        }
        seg[2 * numFiles] = seg[2 * numFiles - 1];
    }
    const uint32_t step = packed ? 2 : 1;
    const uint64_t totalFrames = packed ? (uint64_t)np * frame : table[numFiles];
    const alac_hip_int_source src = {bps, mConfig.bitDepth, 1, 0, 1, C};
    const uint64_t rows = alac_hip_loudness_rows(mConfig.sampleRate, totalFrames, seg.data(), nseg);
    const uint64_t loudWs = alac_hip_loudness_workspace_bytes(mConfig.sampleRate, C, totalFrames, nseg);
    if (loudWs == 0) return mLastStatus = kALAC_ParamError;  // a sample rate the measurement does not take
    std::vector<double> energy((size_t)rows * C);
    std::vector<alac_hip_loudness_report> rep(nseg);
    if (dLoudWs.alloc(loudWs) || dRows.alloc(rows * C * 8ull) || dRep.alloc(nseg * 32ull)) return mLastStatus = kALAC_MemFullError;
    mLastStatus = alac_hip_loudness_int(mCtx, plane, &src, C, mConfig.sampleRate, totalFrames, seg.data(), nseg, dLoudWs.p, loudWs,
                                        (double *)dRows.p, rows, (alac_hip_loudness_report *)dRep.p);
    if (mLastStatus != ALAC_HIP_noErr) return mLastStatus;
    std::vector<alac_hip_true_peak_report> peakRep(outTruePeak ? nseg : 0);
    if (outTruePeak) {
        const uint64_t peakWs = alac_hip_true_peak_workspace_bytes(C, nseg);
        if (dPeakWs.alloc(peakWs) || dPeaks.alloc((uint64_t)nseg * C * 8) || dPeakRep.alloc(nseg * 32ull))
            return mLastStatus = kALAC_MemFullError;
        mLastStatus = alac_hip_true_peak_int(mCtx, plane, &src, C, mConfig.sampleRate, totalFrames, seg.data(), nseg, dPeakWs.p,
                                             peakWs, (double *)dPeaks.p, (alac_hip_true_peak_report *)dPeakRep.p);
        if (mLastStatus != ALAC_HIP_noErr) return mLastStatus;
        if (hipMemcpyAsync(peakRep.data(), dPeakRep.p, nseg * 32ull, hipMemcpyDeviceToHost, st) != hipSuccess)
            return mLastStatus = kALAC_ParamError;
    }
    // only the rows and the reports cross the bus: the PCM stays on the device
    if ((rows && hipMemcpyAsync(energy.data(), dRows.p, rows * C * 8ull, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipMemcpyAsync(rep.data(), dRep.p, nseg * 32ull, hipMemcpyDeviceToHost, st) != hipSuccess)
        return mLastStatus = kALAC_ParamError;
    if ((mLastStatus = alac_hip_synchronize(mCtx)) != ALAC_HIP_noErr) return mLastStatus;
    for (uint32_t j = 0; j < numFiles; j++) {
        const alac_hip_loudness_report &r = rep[step * j];
        outPeak[j] = r.peak;
        if (outTruePeak) outTruePeak[j] = peakRep[step * j].true_peak;
        mLastStatus = alac_hip_loudness_integrated(energy.data() + (size_t)r.first_block * C, r.num_blocks, C,
                                                   mConfig.sampleRate / 10, nullptr, &outLufs[j]);
        if (mLastStatus != ALAC_HIP_noErr) return mLastStatus;
    }
    return mLastStatus = ALAC_noErr;
}

int32_t ALACDecoder::Decode(BitBuffer *bits, uint8_t *sampleBuffer, uint32_t /*numSamples*/, uint32_t numChannels,
                            uint32_t *outNumSamples)
{
    if (!bits || !sampleBuffer || !outNumSamples || numChannels == 0) return kALAC_ParamError;
    if (!(bits->cur < bits->end)) return kALAC_ParamError;  // :615
    const uint32_t n = (uint32_t)(bits->end - bits->cur);
    const uint32_t bpf = mConfig.numChannels * bps_of(mConfig.bitDepth);
    std::vector<uint8_t> pcm((size_t)mConfig.frameLength * bpf);
    uint32_t ns = 0;
    int32_t st = 0;
    int32_t rc = DecodeBatch(bits->cur, &n, 1, pcm.data(), &ns, &st);
    if (rc != ALAC_noErr) return rc;
    if (st != 0) return st;
    memcpy(sampleBuffer, pcm.data(), (size_t)ns * bpf);
    *outNumSamples = ns;
    bits->cur = bits->end;  // the whole packet was consumed
    bits->bitIndex = 0;
    return ALAC_noErr;
}

int32_t ALACDecoder::Decode(BitBuffer *bits, uint32_t numSamples, uint32_t numChannels, uint32_t *outNumSamples,
                            uint32_t /*outBytesPerPacket*/, int X)
{
    if (!bits || !outNumSamples || numChannels == 0 || X < 0) return kALAC_ParamError;
    if (!(bits->cur < bits->end)) return kALAC_ParamError;
    if ((size_t)X != mQueuedSizes.size()) return kALAC_ParamError;  // packets are queued in order
    const size_t n = (size_t)(bits->end - bits->cur);
    mQueued.insert(mQueued.end(), bits->cur, bits->end);
    mQueuedSizes.push_back((uint32_t)n);
    uint32_t ns = peek_num_samples(bits->cur, n, mConfig.frameLength);
    *outNumSamples = ns ? ns : numSamples;
    return ALAC_noErr;
}

void ALACDecoder::fillWriteBuffer(void *deviceSampleBuffer, uint32_t /*numChannels*/, int32_t theOutputPacketBytes,
                                  int /*X*/)
{
    mLastStatus = kALAC_ParamError;
    if (!mCtx || mCookie.empty() || !deviceSampleBuffer || mQueuedSizes.empty()) return;
    const uint32_t bpf = mConfig.numChannels * bps_of(mConfig.bitDepth);
    if ((uint32_t)theOutputPacketBytes != mConfig.frameLength * bpf) return;
    const uint32_t np = (uint32_t)mQueuedSizes.size();
    alac_hip_format fmt = {mConfig.frameLength, mConfig.bitDepth, mConfig.numChannels, mConfig.sampleRate};
    hipStream_t st = (hipStream_t)alac_hip_stream(mCtx);
    alachost::DevStream d;
    alachost::DevBuf dWs, dNs, dSt;
    uint64_t wsBytes = 0;
    // a failed staging step is kALAC_MemFullError here, whichever it is
    if (alachost::upload_stream(mQueued.data(), mQueuedSizes.data(), np, st, d,
                                [](int32_t, const char *, hipError_t) { return (int32_t)kALAC_MemFullError; }) ||
        dWs.alloc(wsBytes = alac_hip_decode_workspace_bytes_stream(&fmt, np, d.total)) || dNs.alloc(np * 4ull) ||
        dSt.alloc(np * 4ull)) {
        mLastStatus = kALAC_MemFullError;
    } else {
        mLastStatus = alac_hip_decode(mCtx, mCookie.data(), (uint32_t)mCookie.size(), (const uint8_t *)d.bytes.p,
                                      (const uint64_t *)d.offs.p, np, dWs.p, wsBytes, (uint8_t *)deviceSampleBuffer,
                                      (uint32_t *)dNs.p, (int32_t *)dSt.p);
        if (mLastStatus == ALAC_HIP_noErr && alac_hip_synchronize(mCtx) != ALAC_HIP_noErr) mLastStatus = kALAC_ParamError;
        // per-packet results: a packet that failed to decode must not pass for audio — its slot in the caller's buffer is
        // zeroed and the first failure becomes the status of the call (what Decode returned for that packet in the
        // reference's per-packet loop, convert-utility/main.cu:719-724)
        if (mLastStatus == ALAC_HIP_noErr) {
            std::vector<int32_t> stv(np, 0);
            if (hipMemcpy(stv.data(), dSt.p, np * 4ull, hipMemcpyDeviceToHost) != hipSuccess) mLastStatus = kALAC_ParamError;
            int32_t first = ALAC_HIP_noErr;
            for (uint32_t i = 0; i < np && mLastStatus == ALAC_HIP_noErr; i++) {
                if (stv[i] == 0) continue;
                if (first == ALAC_HIP_noErr) first = stv[i];
                if (hipMemset((uint8_t *)deviceSampleBuffer + (size_t)i * theOutputPacketBytes, 0,
                              (size_t)theOutputPacketBytes) != hipSuccess)
                    mLastStatus = kALAC_ParamError;
            }
            if (mLastStatus == ALAC_HIP_noErr) mLastStatus = first;
        }
    }
    mQueued.clear();
    mQueuedSizes.clear();
}
