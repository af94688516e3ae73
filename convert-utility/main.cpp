/*
 * alacconvert — drop-in for the reference's convert utility (convert-utility/main.cu:73-852) on the MI355X path.
 *
 *   alacconvert <input wav or caf file> <output caf file>        encode (PCM -> ALAC in CAF)
 *   alacconvert <input caf file> <output wav or caf file>        decode (ALAC in CAF -> PCM)
 *
 * Both produce the bytes the reference produces for the same input.  The codec work goes through the same
 * ALACEncoder / ALACDecoder classes the reference's main() uses (include/alac/), which run on the GPU; this file
 * and container.cpp are plain host C++.
 *
 * Extensions (not in the reference):
 *   <output>.m4a / .mp4 on encode, an MP4 / M4A input on decode: ALAC in an ISO base media file (one 'alac' track, the
 *                                             sample description of ALACMagicCookieDescription.txt:177-216) instead of CAF
 *   --batch <in1> <out1> [<in2> <out2> ...]   convert many files in one GPU batch; every output is identical to a
 *                                             single-file run (each file is one independent chain of packets)
 *   --segment-packets K                       encode only: restart the predictor state every K packets so that
 *                                             one long file spreads over the GPU (valid ALAC, NOT byte-identical
 *                                             to the reference's output, about 1 % larger at K = 1)
 *   --lpc                                     encode only: every packet independent, each channel with predictor
 *                                             coefficients computed from the packet's own PCM where they code smaller
 *                                             (valid ALAC, NOT byte-identical to the reference's output, never larger
 *                                             than --segment-packets 1); mono and stereo
 *   --devices N                               with --batch: the files are dealt round-robin to N GPUs, one context and
 *                                             one host thread per device (replicas: independent files need no exchange
 *                                             between the GPUs, so there is no RCCL here); outputs are unchanged
 *   --verify                                  encode only: decode every encoded group on its own device and compare it with
 *                                             the PCM it was encoded from (alac_hip_verify) before any file is written; on
 *                                             a mismatch name the file, packet and frame, write nothing, exit 1.  The
 *                                             output bytes are those of the same command without --verify
 *   --compare <in.caf|in.m4a> <reference.wav> decode an ALAC file and compare it with a WAV / PCM CAF on the GPU, writing
 *                                             nothing: exit 0 if every frame matches, 1 otherwise (or on an error).  A 32-bit
 *                                             float WAV / CAF reference is compared through the quantization rule at the
 *                                             stream's bit depth; --dither [--dither-seed S] may be added for a file that was
 *                                             encoded with it
 *   --float-bits N                            encode only, N = 16, 20, 24 or 32: the inputs are 32-bit IEEE-float PCM (WAVE
 *                                             format tag 3 or EXTENSIBLE float, CAF lpcm with the float flag, either byte
 *                                             order), quantized on the GPU (alac_hip_encode_float) and encoded at N bits.  The
 *                                             output is the file an integer input holding the quantized samples gives; a
 *                                             clip count is a warning on stderr.  Integer or 64-bit float inputs and
 *                                             --verify are refused
 *   --float-bits auto                         as --float-bits N, with N chosen per file: the smallest of 16, 20, 24, 32 at
 *                                             which the file's floats encode losslessly (alac_hip_float_probe, one call per
 *                                             channel count, one segment per file), printed per file.  A --batch of mixed
 *                                             material comes out as 16-bit and 24-bit streams side by side.  A file that has
 *                                             no such depth (off-grid samples, a sample at or above 1.0, a NaN) is named with
 *                                             its need_bits, over_range and nan counts; nothing is written, exit 1: auto
 *                                             promises lossless, a lossy reduction stays an explicit N.  Not with --dither
 *   --verify-source                           with --float-bits N [--dither [--dither-seed S]]: after a group is encoded, decode
 *                                             its stream on the device and compare it with the FLOAT data of the input files
 *                                             through the quantization rule (alac_hip_verify_float: rounding, saturation,
 *                                             NaN -> 0, the dither of the same seed; every file's frames count from 0) before
 *                                             any file is written; on a mismatch name file, packet and frame, write nothing,
 *                                             exit 1.  --verify is "against the PCM handed to the encoder", --verify-source
 *                                             is "against the float file, through the rule"; a float encode has only the latter.
 *                                             The output bytes are those of the same command without it
 *   --dither [--dither-seed S]                with --float-bits 16, 20 or 24: triangular (TPDF) dither of +-1 LSB in front of
 *                                             the rounding, generated on the GPU (alac_hip_encode_float_dither) from the seed S
 *                                             (decimal or 0x-hex, default 0: two runs give the same file).  Every file's
 *                                             frames count from 0, so a file's output is the same alone, in --batch and
 *                                             with --devices N
 *   --crc <file> [<file> ...]                 print one line per file, "%08x  <frames>  <path>": the CRC-32 (zlib's) of the file's
 *                                             PCM and its sample-frames, and write nothing.  The PCM is what decoding gives, in
 *                                             the layout of the `data` chunk of the WAV `alacconvert <file> out.wav` writes:
 *                                             little-endian, interleaved, 20-bit samples left-justified in 3 bytes.  ALAC files
 *                                             (CAF, M4A) are decoded and hashed on the GPU (ALACDecoder::TestBatch: the PCM never
 *                                             comes back to the host), files of one cookie in one batch; integer PCM files (WAV,
 *                                             CAF) have their sample bytes hashed there (alac_hip_pcm_crc32_host), so a file and
 *                                             its encode print the same value.  Float PCM is refused.  A file with an
 *                                             undecodable packet is named with the packet's index; exit 1.  With --devices N the
 *                                             files are dealt to N GPUs.  No other option
 *   --crc-check <list>                        read lines of that format, compute every file's value again and print
 *                                             "<path>: OK", "<path>: FAILED" or "<path>: FAILED open"; exit 1 if any line
 *                                             failed (the flow of sha256sum -c).  With --devices N; no other option
 *
 * A single chained file is serial by construction: one file runs as one chain of dependent
 * packets; the GPU pays off with --batch or --segment-packets.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "alac_hip.h"

#include "ALACAudioTypes.h"
#include "ALACDecoder.h"
#include "ALACEncoder.h"
#include "container.h"

using alacfile::Bytes;
using alacfile::InputInfo;

namespace {

struct Job {
    std::string in, out;
    Bytes file;
    InputInfo info;
    Bytes result;
    // --float-bits: info describes the integer file of the quantized samples; the floats are at floatPos in `file`
    bool floatIn = false, floatBigEndian = false;
    uint64_t floatPos = 0;
};

void usage()
{
    // main.cu:181-189
    printf("Usage:\n");
    printf("Encode:\n");
    printf("        alacconvert <input wav or caf file> <output caf file>\n");
    printf("Decode:\n");
    printf("        alacconvert <input caf file> <output wav or caf file>\n");
    printf("\n");
    printf("Extensions:\n");
    printf("        alacconvert --batch <in1> <out1> [<in2> <out2> ...]\n");
    printf("        alacconvert --segment-packets K <input wav or caf file> <output caf file>\n");
    printf("        alacconvert --batch --devices N <in1> <out1> [<in2> <out2> ...]\n");
    printf("        alacconvert --lpc [--batch] <input wav or caf file> <output caf or m4a file> ...\n");
    printf("        alacconvert --verify [--batch] [--lpc] ... <input wav or caf file> <output caf or m4a file> ...\n");
    printf("        alacconvert --compare <input caf or m4a file> <reference wav or caf file>\n");
    printf("        alacconvert --float-bits N [--batch] [--lpc] ... <input float wav or caf file> <output caf or m4a file> ...\n");
    printf("        alacconvert --float-bits auto [--batch] [--lpc] [--verify-source] ... <input float wav or caf file> <output caf or m4a file> ...\n");
    printf("            (every file at the smallest of 16, 20, 24, 32 bits at which it is lossless, probed on the GPU; a file that\n");
    printf("             has none is refused; no --dither)\n");
    printf("        alacconvert --float-bits N --dither [--dither-seed S] ... <input float wav or caf file> <output caf or m4a file> ...\n");
    printf("        alacconvert --float-bits N [--dither [--dither-seed S]] --verify-source ... <input float wav or caf file> <output caf or m4a file> ...\n");
    printf("            (--verify checks against the PCM handed to the encoder, --verify-source against the float file through the\n");
    printf("             quantization rule)\n");
    printf("        alacconvert --compare [--dither [--dither-seed S]] <input caf or m4a file> <reference float wav or caf file>\n");
    printf("        alacconvert --crc [--devices N] <wav, caf or m4a file> ...\n");
    printf("            (one line per file: CRC-32 of its PCM, sample-frames, path; ALAC is decoded and hashed on the GPU)\n");
    printf("        alacconvert --crc-check [--devices N] <list written by --crc>\n");
    printf("\n");
}

uint32_t source_bits(uint32_t flag) { return flag == 1 ? 16 : flag == 2 ? 20 : flag == 3 ? 24 : flag == 4 ? 32 : 0; }

AudioFormatDescription alac_format(const InputInfo &in)
{
    // SetOutputFormat, encode branch (main.cu:263-301)
    AudioFormatDescription f;
    memset(&f, 0, sizeof(f));
    f.mFormatID = kALACFormatAppleLossless;
    f.mSampleRate = in.sampleRate;
    f.mFormatFlags = in.bitsPerChannel == 16 ? 1 : in.bitsPerChannel == 20 ? 2 : in.bitsPerChannel == 24 ? 3 : 4;
    f.mFramesPerPacket = kALACDefaultFramesPerPacket;
    f.mChannelsPerFrame = in.channels;
    return f;
}

// ---- encode: all jobs share bit depth and channel count; each file is one segment ----
// --verify: decode the group's stream on `device` and compare it with the PCM it was encoded from; names the first bad
// packet of every file that fails
bool verify_group(std::vector<Job *> &jobs, ALACEncoder &enc, const std::vector<uint32_t> &firstPacket, const Bytes &pcm,
                  const std::vector<uint32_t> &numSamples, const Bytes &stream, const std::vector<uint32_t> &sizes, int device)
{
    const uint32_t np = (uint32_t)sizes.size();
    if (np == 0) return true;
    uint32_t cookieSize = enc.GetMagicCookieSize(jobs[0]->info.channels);
    Bytes cookie(cookieSize, 0);
    enc.GetMagicCookie(cookie.data(), &cookieSize);
    ALACDecoder dec;
    if (device >= 0) dec.SetDevice(device);
    if (dec.Init(cookie.data(), cookieSize, 0) != ALAC_noErr) {
        fprintf(stderr, " Cannot initialise the decoder for --verify\n");
        return false;
    }
    std::vector<uint32_t> firstMismatch(np, 0);
    std::vector<int32_t> status(np, 0);
    uint32_t bad = 0;
    const int32_t rc = dec.VerifyBatch(stream.data(), sizes.data(), np, pcm.data(), numSamples.data(), firstMismatch.data(),
                                       status.data(), &bad);
    if (rc != ALAC_noErr) {
        fprintf(stderr, " Verification failed to run (status %d)\n", rc);
        return false;
    }
    if (bad == 0) return true;
    for (size_t j = 0; j < jobs.size(); j++) {
        const uint32_t p0 = firstPacket[j], p1 = j + 1 < jobs.size() ? firstPacket[j + 1] : np;
        for (uint32_t p = p0; p < p1; p++) {
            if (firstMismatch[p] != 0xffffffffu) {
                fprintf(stderr, " Verify failed: \"%s\" -> \"%s\": packet %u, frame %u (status %d)\n", jobs[j]->in.c_str(),
                        jobs[j]->out.c_str(), p - p0, firstMismatch[p], status[p]);
                break;
            }
        }
    }
    return false;
}

// --dither: TPDF dither with this seed on the float inputs
struct DitherOption {
    bool on = false;
    uint64_t seed = 0;
};

// --verify-source: decode the group's stream on `device` and compare it with the floats it was encoded from, through the rule
// of the float encode (the same dither, every file's frames counted from 0: `origin`); names the first bad packet of every
// file that fails
bool verify_source_group(std::vector<Job *> &jobs, ALACEncoder &enc, const std::vector<uint32_t> &firstPacket,
                         const std::vector<float> &fl, uint32_t ch, const std::vector<uint32_t> &numSamples,
                         const DitherOption &dither, const std::vector<uint64_t> &origin, const Bytes &stream,
                         const std::vector<uint32_t> &sizes, int device)
{
    const uint32_t np = (uint32_t)sizes.size();
    if (np == 0) return true;
    uint32_t cookieSize = enc.GetMagicCookieSize(ch);
    Bytes cookie(cookieSize, 0);
    enc.GetMagicCookie(cookie.data(), &cookieSize);
    ALACDecoder dec;
    if (device >= 0) dec.SetDevice(device);
    if (dec.Init(cookie.data(), cookieSize, 0) != ALAC_noErr) {
        fprintf(stderr, " Cannot initialise the decoder for --verify-source\n");
        return false;
    }
    std::vector<uint32_t> firstMismatch(np, 0);
    std::vector<int32_t> status(np, 0);
    uint32_t bad = 0;
    const int32_t rc = dec.VerifyBatchFloat(stream.data(), sizes.data(), np, fl.data(), 1, ch, numSamples.data(),
                                            dither.on ? ALAC_HIP_DITHER_TPDF : ALAC_HIP_DITHER_NONE, dither.seed, origin.data(),
                                            firstMismatch.data(), status.data(), &bad);
    if (rc != ALAC_noErr) {
        fprintf(stderr, " Verification failed to run (status %d)\n", rc);
        return false;
    }
    if (bad == 0) return true;
    for (size_t j = 0; j < jobs.size(); j++) {
        const uint32_t p0 = firstPacket[j], p1 = j + 1 < jobs.size() ? firstPacket[j + 1] : np;
        for (uint32_t p = p0; p < p1; p++) {
            if (firstMismatch[p] != 0xffffffffu) {
                fprintf(stderr, " Verify failed: \"%s\" -> \"%s\": packet %u, frame %u (status %d)\n", jobs[j]->in.c_str(),
                        jobs[j]->out.c_str(), p - p0, firstMismatch[p], status[p]);
                break;
            }
        }
    }
    return false;
}

// --float-bits auto: every float job gets the smallest depth at which its encode is exactly lossless, found on the GPU
// (alac_hip_float_probe: one call per channel count, one segment per file), and is from then on the integer file of its
// samples at that depth.  A file without such a depth is named with what stands in the way; the run is then refused.
bool probe_float_jobs(std::vector<Job> &jobs, int device)
{
    std::map<uint32_t, std::vector<Job *> > byChannels;
    for (size_t j = 0; j < jobs.size(); j++) byChannels[jobs[j].info.channels].push_back(&jobs[j]);
    ALACEncoder enc;
    if (device >= 0) enc.SetDevice(device);
    bool ok = true;
    for (std::map<uint32_t, std::vector<Job *> >::iterator g = byChannels.begin(); g != byChannels.end(); ++g) {
        const uint32_t ch = g->first;
        std::vector<Job *> &v = g->second;
        std::vector<uint64_t> first(1, 0);  // the files' frames back to back
        for (size_t j = 0; j < v.size(); j++) first.push_back(first.back() + v[j]->info.dataSize / (4ull * ch));
        // interleaved floats: channel_stride 1, frame_stride ch (one float where every file is empty)
        std::vector<float> fl((size_t)(first.back() * ch) + 1, 0.0f);
        for (size_t j = 0; j < v.size(); j++) {
            uint8_t *dst = (uint8_t *)(fl.data() + (size_t)first[j] * ch);
            const uint64_t bytes = (first[j + 1] - first[j]) * ch * sizeof(float);
            memcpy(dst, v[j]->file.data() + v[j]->floatPos, (size_t)bytes);
            if (v[j]->floatBigEndian) alacfile::swap_samples_in_place(dst, bytes, 32);
        }
        std::vector<alac_hip_float_report> reports(v.size());
        const int32_t rc = enc.ProbeFloat(fl.data(), ch, 1, ch, first.back(), first.data(), (uint32_t)v.size(), reports.data());
        if (rc != ALAC_noErr) {
            fprintf(stderr, " Probing the float input failed (status %d)\n", rc);
            return false;
        }
        for (size_t j = 0; j < v.size(); j++) {
            Job &J = *v[j];
            const alac_hip_float_report &r = reports[j];
            const uint32_t depth = alac_hip_float_report_depth(&r);
            if (depth == 0) {
                fprintf(stderr, " --float-bits auto: no lossless bit depth (need_bits %u, over_range %llu, nan %llu): \"%s\"\n",
                        r.need_bits, (unsigned long long)r.over_range, (unsigned long long)r.nan, J.in.c_str());
                ok = false;
                continue;
            }
            printf("Float input is lossless at %u bits: %s\n", depth, J.in.c_str());
            J.info.bitsPerChannel = depth;
            J.info.dataSize = (first[j + 1] - first[j]) * ch * ((depth + 7) >> 3);
        }
    }
    return ok;
}

bool encode_group(std::vector<Job *> &jobs, uint32_t segmentPackets, bool lpc, bool verify, bool verifySource,
                  const DitherOption &dither, int device)
{
    const InputInfo &first = jobs[0]->info;
    const uint32_t bps = (first.bitsPerChannel + 7) >> 3, ch = first.channels;  // 20 bits: 3-byte containers (container.cpp)
    const uint32_t bytesPerFrame = bps * ch, frame = kALACDefaultFramesPerPacket;
    const uint64_t packetBytes = (uint64_t)bytesPerFrame * frame;

    ALACEncoder enc;
    enc.SetFrameSize(frame);
    enc.SetLPCMode(lpc);
    if (dither.on) enc.SetDither(ALAC_HIP_DITHER_TPDF, dither.seed);
    if (device >= 0) enc.SetDevice(device);
    AudioFormatDescription outFmt = alac_format(first);
    if (enc.InitializeEncoder(outFmt, 0) != ALAC_noErr) {
        fprintf(stderr, " Cannot initialise the encoder (status %d)\n", enc.LastStatus());
        return false;
    }

    // packets back to back at the full-packet stride; the reference cuts the payload into full packets plus one
    // partial one (main.cu:476-545) and drops a trailing fraction of a frame (ALACEncoder.cu:984)
    std::vector<uint32_t> numSamples, segFirst(1, 0), firstPacket;
    for (size_t j = 0; j < jobs.size(); j++) {
        const uint64_t n = jobs[j]->info.dataSize;
        const uint64_t full = n / packetBytes, rest = n - full * packetBytes;
        firstPacket.push_back((uint32_t)numSamples.size());
        for (uint64_t p = 0; p < full; p++) numSamples.push_back(frame);
        if (rest) numSamples.push_back((uint32_t)(rest / bytesPerFrame));
        if (segmentPackets == 0) {
            segFirst.push_back((uint32_t)numSamples.size());
        } else {
            for (uint32_t p = firstPacket.back() + segmentPackets; p < numSamples.size(); p += segmentPackets) segFirst.push_back(p);
            segFirst.push_back((uint32_t)numSamples.size());
        }
    }
    // files without payload contribute an empty segment; drop duplicates the segment table cannot hold
    std::vector<uint32_t> segs;
    for (size_t s = 0; s < segFirst.size(); s++)
        if (s == 0 || segFirst[s] != segs.back()) segs.push_back(segFirst[s]);
    const uint32_t np = (uint32_t)numSamples.size();

    const bool floatIn = jobs[0]->floatIn;
    Bytes pcm(floatIn ? 0 : (size_t)np * packetBytes, 0), stream;
    std::vector<uint32_t> sizes(np, 0);
    uint64_t total = 0;
    if (np && floatIn) {
        // interleaved floats at the full-packet stride: channel_stride 1, frame_stride ch
        std::vector<float> fl((size_t)np * frame * ch, 0.0f);
        for (size_t j = 0; j < jobs.size(); j++) {
            Job &J = *jobs[j];
            uint8_t *dst = (uint8_t *)(fl.data() + (size_t)firstPacket[j] * frame * ch);
            const uint64_t bytes = J.info.dataSize / bytesPerFrame * ch * sizeof(float);
            memcpy(dst, J.file.data() + J.floatPos, (size_t)bytes);
            if (J.floatBigEndian) alacfile::swap_samples_in_place(dst, bytes, 32);
        }
        stream.resize((size_t)np * (packetBytes + kALACMaxEscapeHeaderBytes));
        std::vector<uint32_t> clipped(np, 0);
        // every file's frames count from 0: its dither does not depend on the files beside it
        std::vector<uint64_t> origin(np, 0);
        for (size_t j = 0; j < jobs.size(); j++)
            for (uint32_t p = firstPacket[j], p1 = j + 1 < jobs.size() ? firstPacket[j + 1] : np; p < p1; p++)
                origin[p] = (uint64_t)(p - firstPacket[j]) * frame;
        const int32_t rc = enc.EncodeSegmentsFloatAt(fl.data(), 1, ch, numSamples.data(), np, segs.data(),
                                                     (uint32_t)segs.size() - 1, stream.data(), stream.size(), sizes.data(),
                                                     &total, clipped.data(), origin.data());
        if (rc != ALAC_noErr) {
            fprintf(stderr, " Encoding failed (status %d)\n", rc);
            return false;
        }
        for (size_t j = 0; j < jobs.size(); j++) {
            const uint32_t p0 = firstPacket[j], p1 = j + 1 < jobs.size() ? firstPacket[j + 1] : np;
            uint64_t clips = 0;
            for (uint32_t p = p0; p < p1; p++) clips += clipped[p];
            if (clips)
                fprintf(stderr, " Warning: %llu samples clipped to %u bits: \"%s\"\n", (unsigned long long)clips,
                        first.bitsPerChannel, jobs[j]->in.c_str());
        }
        if (verifySource && !verify_source_group(jobs, enc, firstPacket, fl, ch, numSamples, dither, origin, stream, sizes, device))
            return false;
    } else if (np) {
        for (size_t j = 0; j < jobs.size(); j++) {
            Job &J = *jobs[j];
            uint8_t *dst = pcm.data() + (size_t)firstPacket[j] * packetBytes;
            memcpy(dst, J.file.data() + J.info.dataPos, (size_t)J.info.dataSize);
            if (J.info.bigEndianPcm) alacfile::swap_samples_in_place(dst, J.info.dataSize, J.info.bitsPerChannel);
        }
        stream.resize((size_t)np * (packetBytes + kALACMaxEscapeHeaderBytes));
        const int32_t rc = enc.EncodeSegments(pcm.data(), numSamples.data(), np, segs.data(), (uint32_t)segs.size() - 1,
                                              stream.data(), stream.size(), sizes.data(), &total);
        if (rc != ALAC_noErr) {
            fprintf(stderr, " Encoding failed (status %d)\n", rc);
            return false;
        }
        if (verify && !verify_group(jobs, enc, firstPacket, pcm, numSamples, stream, sizes, device)) return false;
    }
    // per file: cookie + container
    std::vector<uint64_t> offs(np + 1, 0);
    for (uint32_t p = 0; p < np; p++) offs[p + 1] = offs[p] + sizes[p];
    for (size_t j = 0; j < jobs.size(); j++) {
        Job &J = *jobs[j];
        ALACEncoder cookieMaker;  // the cookie carries the file's own sample rate
        cookieMaker.SetFrameSize(frame);
        if (device >= 0) cookieMaker.SetDevice(device);
        AudioFormatDescription f = alac_format(J.info);
        cookieMaker.InitializeEncoder(f, 0);
        uint32_t cookieSize = cookieMaker.GetMagicCookieSize(J.info.channels);
        Bytes cookie(cookieSize, 0);
        cookieMaker.GetMagicCookie(cookie.data(), &cookieSize);
        cookie.resize(cookieSize);
        const uint32_t p0 = firstPacket[j], p1 = j + 1 < jobs.size() ? firstPacket[j + 1] : np;
        alacfile::AlacCafParams cp = {J.info.sampleRate, J.info.channels, J.info.bitsPerChannel, frame, J.info.dataSize};
        std::vector<uint32_t> mine(sizes.begin() + p0, sizes.begin() + p1);
        if (alacfile::has_m4a_extension(J.out)) {
            const alacfile::AlacM4aParams mp = {(uint32_t)J.info.sampleRate, J.info.channels, J.info.bitsPerChannel, frame,
                                                J.info.dataSize / bytesPerFrame};
            J.result = alacfile::build_alac_m4a(mp, cookie, mine, stream.data() + offs[p0], offs[p1] - offs[p0]);
        } else {
            J.result = alacfile::build_alac_caf(cp, cookie, mine, stream.data() + offs[p0], offs[p1] - offs[p0]);
        }
    }
    return true;
}

// the packets of an ALAC file back to back
void append_packets(const Job &J, const alacfile::AlacCafContents &c, Bytes &stream, std::vector<uint32_t> &sizes)
{
    uint64_t pos = c.dataPos;
    for (size_t p = 0; p < c.packetBytes.size(); p++) {
        const uint32_t sz = c.packetBytes[p];
        if (!c.packetPos.empty()) pos = c.packetPos[p];  // M4A: chunks need not be contiguous
        stream.insert(stream.end(), J.file.begin() + pos, J.file.begin() + pos + sz);
        sizes.push_back(sz);
        pos += sz;
    }
}

// ---- --compare <alac file> <reference pcm file>: decode and compare on the GPU, write nothing; 0 = identical ----
int compare_files(const std::string &alacPath, const std::string &refPath, const DitherOption &dither)
{
    Job A, R;
    A.in = alacPath;
    R.in = refPath;
    for (Job *J : {&A, &R}) {
        if (!alacfile::read_file(J->in, J->file)) {
            fprintf(stderr, " Cannot open file \"%s\"\n", J->in.c_str());
            return 1;
        }
        const std::string err = alacfile::sniff_input(J->file, J->info, J == &R);  // the reference may be float PCM
        if (!err.empty()) {
            fprintf(stderr, " %s: \"%s\"\n", err.c_str(), J->in.c_str());
            return 1;
        }
    }
    const bool floatRef = !R.info.isAlac && R.info.isFloat;
    if (floatRef && R.info.bitsPerChannel != 32) {
        fprintf(stderr, " %u-bit float reference is not supported (32-bit float): \"%s\"\n", R.info.bitsPerChannel, R.in.c_str());
        return 1;
    }
    if (dither.on && !floatRef) {
        fprintf(stderr, " --compare --dither needs a 32-bit float reference: \"%s\"\n", R.in.c_str());
        return 1;
    }
    if (!A.info.isAlac || R.info.isAlac) {
        fprintf(stderr, " --compare takes an ALAC file (CAF or M4A) and a PCM reference (WAV or CAF)\n");
        return 1;
    }
    alacfile::AlacCafContents c;
    InputInfo again;
    const std::string err = A.info.kind == alacfile::kM4aFile ? alacfile::parse_alac_m4a(A.file, again, c)
                                                              : alacfile::parse_alac_caf(A.file, A.info, c);
    if (!err.empty()) {
        fprintf(stderr, " %s: \"%s\"\n", err.c_str(), A.in.c_str());
        return 1;
    }
    ALACDecoder dec;
    Bytes cookie(c.cookie);
    if (dec.Init(cookie.data(), (uint32_t)cookie.size(), 0) != ALAC_noErr) {
        fprintf(stderr, " Cannot initialise the decoder from the magic cookie\n");
        return 1;
    }
    const uint32_t ch = dec.mConfig.numChannels, bits = dec.mConfig.bitDepth, frame = dec.mConfig.frameLength;
    if (dither.on && bits == 32) {
        fprintf(stderr, " --dither needs a 16-, 20- or 24-bit stream: \"%s\"\n", A.in.c_str());
        return 1;
    }
    if (ch != R.info.channels || (!floatRef && bits != R.info.bitsPerChannel)) {
        printf("Compare: \"%s\" is %u-bit %u-channel, \"%s\" %u-bit %u-channel: different\n", A.in.c_str(), bits, ch,
               R.in.c_str(), R.info.bitsPerChannel, R.info.channels);
        return 1;
    }
    // bytes of one frame of the reference: float32 samples, or the stream's own integer containers
    const uint64_t bytesPerFrame = floatRef ? (uint64_t)ch * 4 : (uint64_t)ch * ((bits + 7) >> 3), packetBytes = bytesPerFrame * frame;
    std::vector<uint32_t> sizes;
    Bytes stream;
    append_packets(A, c, stream, sizes);
    const uint32_t np = (uint32_t)sizes.size();
    // the reference cut into packets as the encoder cuts it: full packets, then one partial packet
    const uint64_t refFrames = R.info.dataSize / bytesPerFrame;
    const uint64_t refPackets = (refFrames + frame - 1) / frame;
    Bytes pcm((size_t)np * packetBytes, 0);
    std::vector<uint32_t> expected(np, 0);
    for (uint32_t p = 0; p < np && p < refPackets; p++) {
        const uint64_t f0 = (uint64_t)p * frame, n = refFrames - f0 < frame ? refFrames - f0 : frame;
        expected[p] = (uint32_t)n;
        memcpy(pcm.data() + (size_t)p * packetBytes, R.file.data() + R.info.dataPos + f0 * bytesPerFrame, (size_t)(n * bytesPerFrame));
        if (R.info.bigEndianPcm)
            alacfile::swap_samples_in_place(pcm.data() + (size_t)p * packetBytes, n * bytesPerFrame, R.info.bitsPerChannel);
    }
    // (a float reference sits in `pcm` as interleaved floats at the full-packet stride: channel stride 1, frame stride ch;
    // one file, so its frames count from 0 as the encode numbered them — no origin table)
    std::vector<uint32_t> firstMismatch(np, 0);
    std::vector<int32_t> status(np, 0);
    uint32_t bad = 0;
    if (np) {
        const int32_t rc =
            floatRef ? dec.VerifyBatchFloat(stream.data(), sizes.data(), np, (const float *)pcm.data(), 1, ch, expected.data(),
                                            dither.on ? ALAC_HIP_DITHER_TPDF : ALAC_HIP_DITHER_NONE, dither.seed, nullptr,
                                            firstMismatch.data(), status.data(), &bad)
                     : dec.VerifyBatch(stream.data(), sizes.data(), np, pcm.data(), expected.data(), firstMismatch.data(),
                                       status.data(), &bad);
        if (rc != ALAC_noErr) {
            fprintf(stderr, " Verification failed to run (status %d)\n", rc);
            return 1;
        }
    }
    for (uint32_t p = 0; p < np && bad; p++) {
        if (firstMismatch[p] != 0xffffffffu) {
            printf("Compare: \"%s\" differs from \"%s\" at packet %u, frame %u (sample-frame %llu, status %d)\n", A.in.c_str(),
                   R.in.c_str(), p, firstMismatch[p], (unsigned long long)((uint64_t)p * frame + firstMismatch[p]), status[p]);
            return 1;
        }
    }
    if (refPackets != np) {
        printf("Compare: \"%s\" has %u packets, \"%s\" makes %llu\n", A.in.c_str(), np, R.in.c_str(),
               (unsigned long long)refPackets);
        return 1;
    }
    printf("Compare: \"%s\" matches \"%s\" (%u packets)\n", A.in.c_str(), R.in.c_str(), np);
    return 0;
}

// ---- decode: jobs with identical cookies decode in one batch ----
bool decode_group(std::vector<Job *> &jobs, const std::vector<alacfile::AlacCafContents> &contents, int device)
{
    const Bytes &cookie = contents[0].cookie;
    ALACDecoder dec;
    if (device >= 0) dec.SetDevice(device);
    Bytes cookieCopy(cookie);
    if (dec.Init(cookieCopy.data(), (uint32_t)cookieCopy.size(), 0) != ALAC_noErr) {
        fprintf(stderr, " Cannot initialise the decoder from the magic cookie\n");
        return false;
    }
    const uint32_t ch = dec.mConfig.numChannels, bits = dec.mConfig.bitDepth, frame = dec.mConfig.frameLength;
    // The 'desc' flag was checked by the caller, but the COOKIE decides what the decoder writes: refuse a cookie whose depth
    // contradicts the file's description.  20 bits: 3-byte samples, left-justified, as the library writes them.
    for (size_t j = 0; j < jobs.size(); j++) {
        if (!(bits == 16 || bits == 20 || bits == 24 || bits == 32) || source_bits(jobs[j]->info.alacSourceFlag) != bits) {
            fprintf(stderr, " Magic cookie bit depth %u does not match the file description: \"%s\"\n", bits, jobs[j]->in.c_str());
            return false;
        }
    }
    const uint32_t bytesPerFrame = ch * ((bits + 7) >> 3);
    std::vector<uint32_t> sizes, firstPacket;
    Bytes stream;
    for (size_t j = 0; j < jobs.size(); j++) {
        firstPacket.push_back((uint32_t)sizes.size());
        append_packets(*jobs[j], contents[j], stream, sizes);
    }
    const uint32_t np = (uint32_t)sizes.size();
    Bytes pcm((size_t)np * frame * bytesPerFrame);
    std::vector<uint32_t> ns(np, 0);
    std::vector<int32_t> status(np, 0);
    if (np) {
        const int32_t rc = dec.DecodeBatch(stream.data(), sizes.data(), np, pcm.data(), ns.data(), status.data());
        if (rc != ALAC_noErr) {
            fprintf(stderr, " Decoding failed (status %d)\n", rc);
            return false;
        }
    }
    for (size_t j = 0; j < jobs.size(); j++) {
        Job &J = *jobs[j];
        const uint32_t p0 = firstPacket[j], p1 = j + 1 < jobs.size() ? firstPacket[j + 1] : np;
        Bytes outPcm;
        for (uint32_t p = p0; p < p1; p++) {
            // main.cu:721-724: numFrames of every packet counts, whatever its status
            const uint8_t *src = pcm.data() + (size_t)p * frame * bytesPerFrame;
            outPcm.insert(outPcm.end(), src, src + (size_t)ns[p] * bytesPerFrame);
        }
        if (alacfile::has_wav_extension(J.out)) {
            if (ch > 2) {
                fprintf(stderr, " Cannot decode more than two channels to WAVE\n");  // main.cu:169-174
                return false;
            }
            J.result = alacfile::build_wave(dec.mConfig.sampleRate, ch, bits, outPcm.data(), outPcm.size());
        } else {
            J.result = alacfile::build_pcm_caf(dec.mConfig.sampleRate, ch, bits, outPcm.data(), outPcm.size());
        }
    }
    return true;
}

// ---- --crc / --crc-check: the CRC-32 of every file's PCM, computed on the GPU; nothing is written ----
struct CrcJob {
    Job job;
    alacfile::AlacCafContents contents;  // ALAC files
    bool opened = false, done = false;
    uint32_t crc = 0;
    uint64_t frames = 0;
};

// ALAC files of one cookie: one TestBatch, one range per file
void crc_alac_group(std::vector<CrcJob *> &jobs, int device)
{
    ALACDecoder dec;
    if (device >= 0) dec.SetDevice(device);
    Bytes cookie(jobs[0]->contents.cookie);
    if (dec.Init(cookie.data(), (uint32_t)cookie.size(), 0) != ALAC_noErr) {
        fprintf(stderr, " Cannot initialise the decoder from the magic cookie: \"%s\"\n", jobs[0]->job.in.c_str());
        return;
    }
    const uint32_t ch = dec.mConfig.numChannels, bits = dec.mConfig.bitDepth;
    const uint32_t bytesPerFrame = ch * ((bits + 7) >> 3);
    std::vector<CrcJob *> take;
    for (size_t j = 0; j < jobs.size(); j++) {  // as decode_group: the cookie decides what the decoder writes
        if (!(bits == 16 || bits == 20 || bits == 24 || bits == 32) || source_bits(jobs[j]->job.info.alacSourceFlag) != bits)
            fprintf(stderr, " Magic cookie bit depth %u does not match the file description: \"%s\"\n", bits, jobs[j]->job.in.c_str());
        else
            take.push_back(jobs[j]);
    }
    if (take.empty()) return;
    std::vector<uint32_t> sizes, firstPacket;
    Bytes stream;
    for (size_t j = 0; j < take.size(); j++) {
        firstPacket.push_back((uint32_t)sizes.size());
        append_packets(take[j]->job, take[j]->contents, stream, sizes);
    }
    const uint32_t np = (uint32_t)sizes.size();
    firstPacket.push_back(np);
    std::vector<alac_hip_pcm_digest> digests(take.size());
    std::vector<uint32_t> frames(np, 0);
    std::vector<int32_t> status(np, 0);
    const int32_t rc = dec.TestBatch(stream.data(), sizes.data(), np, firstPacket.data(), (uint32_t)take.size(), digests.data(),
                                     frames.data(), status.data());
    if (rc != ALAC_noErr) {
        fprintf(stderr, " Decoding failed (status %d): \"%s\"\n", rc, take[0]->job.in.c_str());
        return;
    }
    for (size_t j = 0; j < take.size(); j++) {
        CrcJob &J = *take[j];
        bool good = true;
        for (uint32_t p = firstPacket[j]; p < firstPacket[j + 1] && good; p++) {
            if (status[p] != 0) {
                fprintf(stderr, " Cannot decode packet %u (status %d): \"%s\"\n", p - firstPacket[j], status[p], J.job.in.c_str());
                good = false;
            }
        }
        if (!good) continue;
        J.crc = digests[j].crc32;
        J.frames = digests[j].bytes / bytesPerFrame;
        J.done = true;
    }
}

// integer PCM files: the sample bytes of all of them staged in one buffer, one range per file
void crc_pcm_group(std::vector<CrcJob *> &jobs, int device)
{
    std::vector<uint64_t> ranges;
    Bytes pcm;
    for (size_t j = 0; j < jobs.size(); j++) {
        const InputInfo &in = jobs[j]->job.info;
        const uint64_t bytesPerFrame = (uint64_t)in.channels * ((in.bitsPerChannel + 7) >> 3);
        // whole frames only: the encoder drops a trailing fraction of a frame (ALACEncoder.cu:984)
        const uint64_t bytes = in.dataSize / bytesPerFrame * bytesPerFrame;
        ranges.push_back(pcm.size()), ranges.push_back(bytes);
        jobs[j]->frames = bytes / bytesPerFrame;
        pcm.insert(pcm.end(), jobs[j]->job.file.begin() + in.dataPos, jobs[j]->job.file.begin() + in.dataPos + bytes);
        if (in.bigEndianPcm) alacfile::swap_samples_in_place(pcm.data() + pcm.size() - bytes, bytes, in.bitsPerChannel);
    }
    alac_hip_ctx *ctx = nullptr;
    const char *dev = getenv("ALAC_HIP_DEVICE");
    if (alac_hip_create(&ctx, device >= 0 ? device : (dev ? atoi(dev) : 0), nullptr) != ALAC_HIP_noErr) {
        fprintf(stderr, " Cannot create a GPU context\n");
        return;
    }
    std::vector<alac_hip_pcm_digest> digests(jobs.size());
    const int32_t rc = alac_hip_pcm_crc32_host(ctx, pcm.data(), pcm.size(), ranges.data(), (uint32_t)jobs.size(), digests.data());
    if (rc != ALAC_HIP_noErr) fprintf(stderr, " Hashing failed (status %d): %s\n", rc, alac_hip_last_error(ctx));
    alac_hip_destroy(ctx);
    if (rc != ALAC_HIP_noErr) return;
    for (size_t j = 0; j < jobs.size(); j++) {
        jobs[j]->crc = digests[j].crc32;
        jobs[j]->done = true;
    }
}

// opens, sniffs and hashes every job; a job that cannot be done is named on stderr and keeps done == false
void crc_run(std::vector<CrcJob> &jobs, uint32_t devices)
{
    std::map<std::string, std::vector<CrcJob *> > groups;  // ALAC files by cookie ("D..."), all PCM files ("P")
    for (size_t j = 0; j < jobs.size(); j++) {
        CrcJob &J = jobs[j];
        if (!alacfile::read_file(J.job.in, J.job.file)) {
            fprintf(stderr, " Cannot open file \"%s\"\n", J.job.in.c_str());
            continue;
        }
        J.opened = true;
        InputInfo &info = J.job.info;
        std::string err = alacfile::sniff_input(J.job.file, info, true);
        if (err.empty() && info.isAlac) {
            InputInfo again;
            err = info.kind == alacfile::kM4aFile ? alacfile::parse_alac_m4a(J.job.file, again, J.contents)
                                                  : alacfile::parse_alac_caf(J.job.file, info, J.contents);
        }
        if (!err.empty()) {
            fprintf(stderr, " %s: \"%s\"\n", err.c_str(), J.job.in.c_str());
            continue;
        }
        if (!info.isAlac && info.isFloat) {
            fprintf(stderr, " --crc does not take float PCM: \"%s\"\n", J.job.in.c_str());
            continue;
        }
        const uint32_t b = info.bitsPerChannel;
        if (!info.isAlac && ((b != 16 && b != 20 && b != 24 && b != 32) || info.channels < 1 || info.channels > 8)) {
            fprintf(stderr, " File \"%s\'s\" data format is of an unsupported type\n", J.job.in.c_str());
            continue;
        }
        groups[info.isAlac ? "D" + std::string(J.contents.cookie.begin(), J.contents.cookie.end()) : std::string("P")].push_back(&J);
    }
    // the files of every group dealt round-robin to the workers, as the conversions are
    struct Work {
        std::vector<CrcJob *> jobs;
        bool alac;
    };
    const uint32_t workers = devices ? devices : 1;
    const int32_t visible = devices ? alac_hip_device_count() : 1;
    std::vector<std::vector<Work> > perWorker(workers);
    uint32_t next = 0;
    for (std::map<std::string, std::vector<CrcJob *> >::iterator g = groups.begin(); g != groups.end(); ++g) {
        std::vector<Work> parts(workers);
        for (size_t j = 0; j < g->second.size(); j++) {
            Work &w = parts[(next + j) % workers];
            w.alac = g->second[j]->job.info.isAlac;
            w.jobs.push_back(g->second[j]);
        }
        for (uint32_t k = 0; k < workers; k++)
            if (!parts[k].jobs.empty()) perWorker[k].push_back(parts[k]);
        next = (uint32_t)((next + g->second.size()) % workers);
    }
    auto run = [&](uint32_t k) {
        const int device = devices ? (int)(k % (uint32_t)visible) : -1;
        for (size_t i = 0; i < perWorker[k].size(); i++)
            (perWorker[k][i].alac ? crc_alac_group : crc_pcm_group)(perWorker[k][i].jobs, device);
    };
    if (workers == 1) {
        run(0);
    } else {
        std::vector<std::thread> threads;
        for (uint32_t k = 0; k < workers; k++) threads.emplace_back(run, k);
        for (size_t k = 0; k < threads.size(); k++) threads[k].join();
    }
}

// --devices N as the conversions take it
bool crc_devices_ok(uint32_t devices)
{
    if (!devices) return true;
    const int32_t have = alac_hip_device_count();
    if (have < 1 || ((int32_t)devices > have && !getenv("ALACCONVERT_SHARE_DEVICES"))) {
        fprintf(stderr, " --devices %u: only %d GPU(s) visible\n", devices, have);
        return false;
    }
    return true;
}

int crc_files(const std::vector<std::string> &paths, uint32_t devices)
{
    if (!crc_devices_ok(devices)) return 1;
    std::vector<CrcJob> jobs(paths.size());
    for (size_t j = 0; j < jobs.size(); j++) jobs[j].job.in = paths[j];
    crc_run(jobs, devices);
    int rc = 0;
    for (size_t j = 0; j < jobs.size(); j++) {
        if (jobs[j].done) printf("%08x  %llu  %s\n", jobs[j].crc, (unsigned long long)jobs[j].frames, jobs[j].job.in.c_str());
        else rc = 1;
    }
    return rc;
}

int crc_check(const std::string &listPath, uint32_t devices)
{
    if (!crc_devices_ok(devices)) return 1;
    std::ifstream list(listPath.c_str());
    if (!list) {
        fprintf(stderr, " Cannot open file \"%s\"\n", listPath.c_str());
        return 1;
    }
    std::vector<CrcJob> jobs;
    std::vector<uint32_t> wantCrc;
    std::vector<uint64_t> wantFrames;
    int rc = 0;
    std::string line;
    for (unsigned n = 1; std::getline(list, line); n++) {
        if (line.empty()) continue;
        // "%08x  <frames>  <path>": the path is everything behind the second pair of blanks
        const size_t a = line.find("  "), b = a == std::string::npos ? a : line.find("  ", a + 2);
        char *endCrc = nullptr, *endFrames = nullptr;
        const unsigned long crc = strtoul(line.c_str(), &endCrc, 16);
        const unsigned long long frames = a == std::string::npos ? 0 : strtoull(line.c_str() + a + 2, &endFrames, 10);
        if (a != 8 || b == std::string::npos || b + 2 >= line.size() || endCrc != line.c_str() + a || endFrames != line.c_str() + b) {
            fprintf(stderr, " %s: line %u is not \"<crc32>  <frames>  <path>\"\n", listPath.c_str(), n);
            rc = 1;
            continue;
        }
        jobs.push_back(CrcJob());
        jobs.back().job.in = line.substr(b + 2);
        wantCrc.push_back((uint32_t)crc);
        wantFrames.push_back(frames);
    }
    crc_run(jobs, devices);
    for (size_t j = 0; j < jobs.size(); j++) {
        const bool ok = jobs[j].done && jobs[j].crc == wantCrc[j] && jobs[j].frames == wantFrames[j];
        printf("%s: %s\n", jobs[j].job.in.c_str(), ok ? "OK" : jobs[j].opened ? "FAILED" : "FAILED open");
        if (!ok) rc = 1;
    }
    return rc;
}

}  // namespace

int main(int argc, char *argv[])
{
    std::vector<std::string> files;
    bool batch = false, lpc = false, verify = false, verifySource = false, compare = false, malformed = argc < 2;
    uint32_t segmentPackets = 0, devices = 0, floatBits = 0;
    bool crc = false;
    std::string crcList;  // --crc-check <list>
    bool floatAuto = false;  // --float-bits auto: floatBits stays 0, every file gets its own depth from the probe
    DitherOption dither;
    for (int i = 1; i < argc && !malformed; i++) {
        const std::string a = argv[i];
        if (a == "-h") {
            malformed = true;
        } else if (a == "--batch") {
            batch = true;
        } else if (a == "--lpc") {
            lpc = true;
        } else if (a == "--verify") {
            verify = true;
        } else if (a == "--verify-source") {
            verifySource = true;
        } else if (a == "--compare") {
            compare = true;
        } else if (a == "--crc") {
            crc = true;
        } else if (a == "--crc-check" && i + 1 < argc) {
            crcList = argv[++i];
            if (crcList.empty()) malformed = true;
        } else if (a == "--segment-packets" && i + 1 < argc) {
            segmentPackets = (uint32_t)strtoul(argv[++i], nullptr, 10);
            if (segmentPackets == 0) malformed = true;
        } else if (a == "--float-bits" && i + 1 < argc) {
            if (std::string(argv[i + 1]) == "auto") {
                floatAuto = true, floatBits = 0, i++;
            } else {
                floatAuto = false;
                floatBits = (uint32_t)strtoul(argv[++i], nullptr, 10);
                if (floatBits != 16 && floatBits != 20 && floatBits != 24 && floatBits != 32) malformed = true;
            }
        } else if (a == "--dither") {
            dither.on = true;
        } else if (a == "--dither-seed" && i + 1 < argc) {
            char *end = nullptr;
            dither.seed = strtoull(argv[++i], &end, 0);  // decimal or 0x-hex
            if (end == argv[i] || *end) malformed = true;
        } else if (a == "--devices" && i + 1 < argc) {
            devices = (uint32_t)strtoul(argv[++i], nullptr, 10);
            if (devices == 0) malformed = true;
        } else if (!a.empty() && a[0] == '-') {
            printf("unknown option: %s\n", a.c_str());  // main.cu:92-96
            malformed = true;
        } else {
            files.push_back(a);
        }
    }
    // --crc and --crc-check stand alone (but --devices N): any number of inputs resp. one list, no output files
    const bool crcMode = crc || !crcList.empty();
    if (!malformed && crcMode &&
        (batch || lpc || verify || verifySource || compare || segmentPackets || floatBits || floatAuto || dither.on ||
         (crc && !crcList.empty()) || (crc ? files.empty() : !files.empty())))
        malformed = true;
    if (!malformed && !crcMode && (files.size() < 2 || (files.size() & 1) || (!batch && files.size() != 2))) malformed = true;
    if (!malformed && !crcMode && devices && !batch) malformed = true;  // one file is one serial chain: nothing to deal out
    // --compare stands alone: two files, no other option
    // (but --dither [--dither-seed S], for a float reference of a file that was encoded with it)
    const bool floatInput = floatBits != 0 || floatAuto;
    if (!malformed && compare && (batch || lpc || verify || verifySource || segmentPackets || devices || floatInput)) malformed = true;
    if (malformed) {
        usage();
        return 1;
    }
    if (crc) return crc_files(files, devices);
    if (!crcList.empty()) return crc_check(crcList, devices);
    if (compare) return compare_files(files[0], files[1], dither);
    if (dither.on && floatBits != 16 && floatBits != 20 && floatBits != 24) {  // auto promises lossless: no dither there
        fprintf(stderr, " --dither needs --float-bits 16, 20 or 24\n");
        usage();
        return 1;
    }
    if (verifySource && !floatInput) {
        fprintf(stderr, " --verify-source needs float input (--float-bits N); --verify checks an integer encode: \"%s\"\n", files[0].c_str());
        return 1;
    }
    if (floatInput && verify) {
        fprintf(stderr, " --verify does not take float input (--float-bits): \"%s\"\n", files[0].c_str());
        return 1;
    }

    std::vector<Job> jobs(files.size() / 2);
    for (size_t j = 0; j < jobs.size(); j++) {
        Job &J = jobs[j];
        J.in = files[2 * j];
        J.out = files[2 * j + 1];
        if (!alacfile::read_file(J.in, J.file)) {
            fprintf(stderr, " Cannot open file \"%s\"\n", J.in.c_str());
            return 1;
        }
        printf("Input file: %s\n", J.in.c_str());
        printf("Output file: %s\n", J.out.c_str());
        const std::string err = alacfile::sniff_input(J.file, J.info, floatInput);
        if (!err.empty()) {
            fprintf(stderr, " %s: \"%s\"\n", err.c_str(), J.in.c_str());
            return 1;
        }
        if (floatInput) {
            if (!J.info.isFloat) {
                fprintf(stderr, " --float-bits takes float PCM input, not integer PCM or ALAC: \"%s\"\n", J.in.c_str());
                return 1;
            }
            if (J.info.bitsPerChannel != 32 || J.info.channels < 1 || J.info.channels > 8) {
                fprintf(stderr, " %u-bit %u-channel float input is not supported (32-bit float, 1 to 8 channels): \"%s\"\n",
                        J.info.bitsPerChannel, J.info.channels, J.in.c_str());
                return 1;
            }
            // from here on the file is the integer file of its quantized samples; the floats stay where they are
            const uint64_t frames = J.info.dataSize / (4ull * J.info.channels);
            J.floatIn = true;
            J.floatPos = J.info.dataPos;
            J.floatBigEndian = J.info.bigEndianPcm;
            J.info.isFloat = J.info.bigEndianPcm = false;
            // (auto: 32 bits until probe_float_jobs below has the file's own depth)
            J.info.bitsPerChannel = floatAuto ? 32 : floatBits;
            J.info.dataSize = frames * J.info.channels * ((J.info.bitsPerChannel + 7) >> 3);
        }
        if (!J.info.isAlac) {
            const uint32_t b = J.info.bitsPerChannel;
            if ((b != 16 && b != 20 && b != 24 && b != 32) || J.info.channels < 1 || J.info.channels > 8) {  // kALACMaxChannels
                fprintf(stderr, " File \"%s\'s\" data format is of an unsupported type\n", J.in.c_str());
                return 1;
            }
        }
    }

    if (floatAuto && !probe_float_jobs(jobs, devices ? 0 : -1)) return 1;

    // group: encode jobs by (depth, channels); decode jobs by cookie
    std::map<std::string, std::vector<Job *> > groups;
    for (size_t j = 0; j < jobs.size(); j++) {
        Job &J = jobs[j];
        std::string key;
        if (J.info.isAlac) {
            alacfile::AlacCafContents c;
            InputInfo again;
            const std::string err = J.info.kind == alacfile::kM4aFile ? alacfile::parse_alac_m4a(J.file, again, c)
                                                                      : alacfile::parse_alac_caf(J.file, J.info, c);
            if (!err.empty()) {
                fprintf(stderr, " %s: \"%s\"\n", err.c_str(), J.in.c_str());
                return 1;
            }
            key = "D" + std::string(c.cookie.begin(), c.cookie.end());
        } else {
            char buf[64];
            snprintf(buf, sizeof(buf), "E%u/%u", J.info.bitsPerChannel, J.info.channels);
            key = buf;
        }
        groups[key].push_back(&J);
    }
    // one unit of work = the jobs of one group that one device takes
    struct Work {
        std::vector<Job *> jobs;
        std::vector<alacfile::AlacCafContents> contents;
        bool decode;
    };
    uint32_t workers = 1;
    int firstDevice = -1;  // -1: the classes' default (ALAC_HIP_DEVICE or 0), the single-device behaviour of every round before
    if (devices) {
        const int32_t have = alac_hip_device_count();
        // ALACCONVERT_SHARE_DEVICES=1 (tests on a one-GPU box): the N workers run side by side on the devices there are
        const bool share = getenv("ALACCONVERT_SHARE_DEVICES") != nullptr;
        if (have < 1 || ((int32_t)devices > have && !share)) {
            fprintf(stderr, " --devices %u: only %d GPU(s) visible\n", devices, have);
            return 1;
        }
        workers = devices;
        firstDevice = 0;
    }
    std::vector<std::vector<Work> > perWorker(workers);
    const int32_t visible = devices ? alac_hip_device_count() : 1;
    uint32_t next = 0;
    for (std::map<std::string, std::vector<Job *> >::iterator g = groups.begin(); g != groups.end(); ++g) {
        std::vector<Job *> &v = g->second;
        const bool dec = v[0]->info.isAlac;
        std::vector<Work> parts(workers);
        for (size_t j = 0; j < v.size(); j++) {
            Work &w = parts[(next + j) % workers];  // files dealt round-robin, continuing where the last group stopped
            w.decode = dec;
            w.jobs.push_back(v[j]);
            if (dec) {
                w.contents.push_back(alacfile::AlacCafContents());
                if (v[j]->info.kind == alacfile::kM4aFile) {
                    InputInfo again;
                    alacfile::parse_alac_m4a(v[j]->file, again, w.contents.back());
                } else {
                    alacfile::parse_alac_caf(v[j]->file, v[j]->info, w.contents.back());
                }
            }
        }
        for (uint32_t k = 0; k < workers; k++)
            if (!parts[(next + k) % workers].jobs.empty()) perWorker[(next + k) % workers].push_back(parts[(next + k) % workers]);
        next = (uint32_t)((next + v.size()) % workers);
    }
    std::vector<int> ok(workers, 1);
    auto run = [&](uint32_t k) {
        const int device = firstDevice < 0 ? -1 : (int)(k % (uint32_t)visible);
        for (size_t i = 0; i < perWorker[k].size() && ok[k]; i++) {
            Work &w = perWorker[k][i];
            ok[k] = w.decode ? decode_group(w.jobs, w.contents, device) : encode_group(w.jobs, segmentPackets, lpc, verify, verifySource, dither, device);
        }
    };
    if (workers == 1) {
        run(0);
    } else {
        // one host thread and one context per device; nothing is shared between them (every Job belongs to one Work)
        std::vector<std::thread> threads;
        for (uint32_t k = 0; k < workers; k++) threads.emplace_back(run, k);
        for (size_t k = 0; k < threads.size(); k++) threads[k].join();
    }
    for (uint32_t k = 0; k < workers; k++)
        if (!ok[k]) return 1;
    for (size_t j = 0; j < jobs.size(); j++) {
        if (!alacfile::write_file(jobs[j].out, jobs[j].result)) {
            fprintf(stderr, " Cannot open file \"%s\"\n", jobs[j].out.c_str());
            return 1;
        }
    }
    return 0;
}
