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
 *   --bits N [--dither [--dither-seed S]]     encode only, N = 16, 20, 24 or 32: the integer PCM inputs (WAV, PCM CAF) are converted
 *                                             to N bits on the GPU by the integer rule of alac_hip.h (alac_hip_pcm_requantize_host:
 *                                             widened exactly, or reduced with round half to even and, with --dither, TPDF dither;
 *                                             every file's frames count from 0) and encoded as files of N bits.  The source of a
 *                                             file: containers of its bytes per sample, its depth significant, a 20-bit file
 *                                             left-justified in 3 bytes.  The output is the file an integer input holding the
 *                                             converted samples gives; a clip count is a warning on stderr; --verify checks
 *                                             against the converted PCM.  --dither needs N below every input's depth.  ALAC and
 *                                             float inputs, --float-bits, --compare, --crc and --crc-check are refused
 *   --bits auto                               as --bits N, with N chosen per file: the smallest of 16, 20, 24, 32 that holds the
 *                                             file's samples exactly (alac_hip_int_probe: one call per depth and channel count, one
 *                                             segment per file), printed per file, with "channels identical" for a stereo file
 *                                             whose channels are.  A 24-bit file of 16-bit samples comes out as the 16-bit
 *                                             file.  Not with --dither
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
 *   --loudness [--devices N] <file> [<file> ...]  print one line per file, "%.2f LUFS  %.2f dBFS  <frames>  <path>": the integrated
 *                                             loudness (ITU-R BS.1770, the value of ReplayGain 2.0 and EBU R128), the sample
 *                                             peak and the sample-frames, "-inf" where there is no value (silence, a file
 *                                             shorter than 400 ms).  ALAC files (CAF, M4A) are decoded on the GPU and measured
 *                                             where they lie (ALACDecoder::LoudnessBatch); integer PCM files go through
 *                                             alac_hip_loudness_int_host, float PCM files through alac_hip_loudness_float_host.
 *                                             Files above two channels are weighted by the layout tag their encode would
 *                                             carry.  A file that cannot be measured (an undecodable packet, a sample rate
 *                                             that is not a multiple of 10 in 8 000 .. 384 000) is named on stderr and the exit
 *                                             status is 1.  No other option is accepted but --true-peak.
 *   --loudness --true-peak [--devices N] <file> ...  the same lines with the true peak (ITU-R BS.1770-4 annex 2, the peak
 *                                             ReplayGain 2.0 and EBU R128 mean) in a column of its own,
 *                                             "%.2f LUFS  %.2f dBFS  %.2f dBTP  <frames>  <path>".  ALAC files go through
 *                                             ALACDecoder::LoudnessTruePeakBatch (both measurements on the one decoded plane),
 *                                             PCM files through alac_hip_true_peak_int_host / _float_host as well.
 *                                             --true-peak without --loudness is refused with the usage text.
 *   --rate R [--float-bits N] [--dither [--dither-seed S]] [--batch] [--devices N]
 *                                             encode only: integer and 32-bit float PCM inputs are converted to R Hz on the GPU
 *                                             (alac_hip_resample_int / _float, the windowed-sinc rule of include/alac_hip.h: each
 *                                             file one segment, the files of one rate, channel count and source format in one
 *                                             call), and the floats are quantized to N bits and encoded as --float-bits N
 *                                             encodes float input; the output's header carries R.  N defaults to an integer
 *                                             input's own depth; a float input needs --float-bits N.  A file already at R is
 *                                             encoded as without --rate and named on stderr; an output peak above full scale is
 *                                             a warning on stderr.  Refused with the usage text: --bits, --float-bits auto,
 *                                             --verify, --verify-source, --compare, the modes that only print, ALAC inputs, and
 *                                             a pair of rates the call does not take
 *   --crc-check <list>                        read lines of that format, compute every file's value again and print
 *                                             "<path>: OK", "<path>: FAILED" or "<path>: FAILED open"; exit 1 if any line
 *                                             failed (the flow of sha256sum -c).  With --devices N; no other option
 *
 * A single chained file is serial by construction: one file runs as one chain of dependent
 * packets; the GPU pays off with --batch or --segment-packets.
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "alac_hip.h"

#include "ALACAudioTypes.h"
#include "ALACDecoder.h"
#include "ALACEncoder.h"
#include "container.h"
#include "plan.h"

using alacfile::Bytes;
using alacfile::InputInfo;
using plan::bytes_per_sample;
using plan::Options;

namespace {

struct Job {
    std::string in, out;
    Bytes file;
    InputInfo info;
    alacfile::AlacCafContents contents;  // ALAC inputs: the cookie and the packets (parse_alac)
    Bytes result;
    // --float-bits: info describes the integer file of the quantized samples; the floats are at floatPos in `file`
    bool floatIn = false, floatBigEndian = false;
    uint64_t floatPos = 0;
    // --rate: the file is resampled from srcRate (0: not resampled); afterwards info describes the integer file of the
    // quantized samples at the new rate, and the floats, interleaved, are in `resampled` instead of `file`
    uint32_t srcRate = 0;
    bool srcFloat = false;
    std::vector<float> resampled;
    // --bits: info describes the integer file of the converted samples; the source's containers, srcBits deep, are at srcPos
    bool intConv = false, srcBigEndian = false;
    uint32_t srcBits = 0;
    uint64_t srcPos = 0, srcFrames = 0;
    // --crc / --crc-check: done only if the file could be hashed
    bool opened = false, done = false;
    uint32_t crc = 0;
    uint64_t crcFrames = 0;
    // --loudness (with done and crcFrames): the integrated loudness in LUFS and the sample peak, 1.0 = full scale; with
    // --true-peak the true peak as well
    double lufs = 0.0, peak = 0.0, truePeak = 0.0;
};
typedef std::map<std::string, std::vector<Job *> > Groups;  // files that go through the GPU in one call

uint32_t source_bits(uint32_t flag) { return flag == 1 ? 16 : flag == 2 ? 20 : flag == 3 ? 24 : flag == 4 ? 32 : 0; }
uint64_t frame_bytes(const InputInfo &in) { return (uint64_t)in.channels * bytes_per_sample(in.bitsPerChannel); }
// ALAC files of one cookie decode in one call
std::string cookie_key(const Job &J) { return "D" + std::string(J.contents.cookie.begin(), J.contents.cookie.end()); }

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

// ---- a file into its Job; whatever stands in the way is said on stderr ----
bool read_job(Job &J)
{
    if (alacfile::read_file(J.in, J.file)) return true;
    fprintf(stderr, " Cannot open file \"%s\"\n", J.in.c_str());
    return false;
}

// the diagnostic of a sniffer or parser, if it gave one
bool refused(const std::string &err, const Job &J)
{
    if (!err.empty()) fprintf(stderr, " %s: \"%s\"\n", err.c_str(), J.in.c_str());
    return !err.empty();
}

// cookie and packet table of an ALAC file (sniff_input has filled J.info)
std::string parse_alac(Job &J)
{
    InputInfo again;
    return J.info.kind == alacfile::kM4aFile ? alacfile::parse_alac_m4a(J.file, again, J.contents)
                                             : alacfile::parse_alac_caf(J.file, J.info, J.contents);
}

// an integer PCM file the encoder takes (kALACMaxChannels)
bool pcm_format_ok(const Job &J)
{
    if (plan::pcm_depth_ok(J.info.bitsPerChannel) && J.info.channels >= 1 && J.info.channels <= 8) return true;
    fprintf(stderr, " File \"%s\'s\" data format is of an unsupported type\n", J.in.c_str());
    return false;
}

// the float payload of a --float-bits input, `frames` interleaved frames of it, in host byte order
void stage_floats(const Job &J, uint64_t frames, float *dst)
{
    const uint64_t bytes = frames * J.info.channels * sizeof(float);
    if (J.srcRate) {
        memcpy(dst, J.resampled.data(), (size_t)bytes);
        return;
    }
    memcpy(dst, J.file.data() + J.floatPos, (size_t)bytes);
    if (J.floatBigEndian) alacfile::swap_samples_in_place((uint8_t *)dst, bytes, 32);
}

// how the containers of a --bits input lie once staged: interleaved, the file's bytes per sample each, its depth significant
// (a 20-bit file is left-justified in 3 bytes; the other depths fill their containers)
alac_hip_int_source int_source_of(const Job &J)
{
    return alac_hip_int_source{bytes_per_sample(J.srcBits), J.srcBits, 1, 0, 1, J.info.channels};
}

// the payload of a --bits input, `frames` interleaved frames of it, little-endian
void stage_source(const Job &J, uint64_t frames, uint8_t *dst)
{
    const uint64_t bytes = frames * J.info.channels * bytes_per_sample(J.srcBits);
    memcpy(dst, J.file.data() + J.srcPos, (size_t)bytes);
    if (J.srcBigEndian) alacfile::swap_samples_in_place(dst, bytes, J.srcBits);
}

// the packets of an ALAC file back to back
void append_packets(const Job &J, Bytes &stream, std::vector<uint32_t> &sizes)
{
    const alacfile::AlacCafContents &c = J.contents;
    uint64_t pos = c.dataPos;
    for (size_t p = 0; p < c.packetBytes.size(); p++) {
        const uint32_t sz = c.packetBytes[p];
        if (!c.packetPos.empty()) pos = c.packetPos[p];  // M4A: chunks need not be contiguous
        stream.insert(stream.end(), J.file.begin() + pos, J.file.begin() + pos + sz);
        sizes.push_back(sz);
        pos += sz;
    }
}

// ... of several files; returns every file's first packet, and the packet count behind the last
std::vector<uint32_t> gather_packets(const std::vector<Job *> &jobs, Bytes &stream, std::vector<uint32_t> &sizes)
{
    std::vector<uint32_t> firstPacket;
    for (size_t j = 0; j < jobs.size(); j++) {
        firstPacket.push_back((uint32_t)sizes.size());
        append_packets(*jobs[j], stream, sizes);
    }
    firstPacket.push_back((uint32_t)sizes.size());
    return firstPacket;
}

// ---- decoders ----
bool open_decoder(ALACDecoder &dec, const Bytes &cookie, int device)
{
    if (device >= 0) dec.SetDevice(device);
    Bytes copy(cookie);
    return dec.Init(copy.data(), (uint32_t)copy.size(), 0) == ALAC_noErr;
}

// The 'desc' flag was checked by the sniffer, but the COOKIE decides what the decoder writes: refuse a cookie whose depth
// contradicts the file's description.  20 bits: 3-byte samples, left-justified, as the library writes them.
bool cookie_matches_description(uint32_t bits, const Job &J)
{
    if (plan::pcm_depth_ok(bits) && source_bits(J.info.alacSourceFlag) == bits) return true;
    fprintf(stderr, " Magic cookie bit depth %u does not match the file description: \"%s\"\n", bits, J.in.c_str());
    return false;
}

// what a verify batch says of every packet: the first frame that differs (0xffffffff: none) and the decode status
struct Verdict {
    std::vector<uint32_t> firstMismatch;
    std::vector<int32_t> status;
    uint32_t bad = 0;
    explicit Verdict(uint32_t np) : firstMismatch(np, 0), status(np, 0) {}
    bool ran(int32_t rc) const
    {
        if (rc != ALAC_noErr) fprintf(stderr, " Verification failed to run (status %d)\n", rc);
        return rc == ALAC_noErr;
    }
    // the first packet of [p0, p1) that differs; p1 if none does
    uint32_t first_bad(uint32_t p0, uint32_t p1) const
    {
        while (p0 < p1 && firstMismatch[p0] == 0xffffffffu) p0++;
        return p0;
    }
};

// names the first bad packet of every file that fails
void report_mismatches(const std::vector<Job *> &jobs, const std::vector<uint32_t> &firstPacket, const Verdict &v)
{
    for (size_t j = 0; j < jobs.size(); j++) {
        const uint32_t p0 = firstPacket[j], p = v.first_bad(p0, firstPacket[j + 1]);
        if (p < firstPacket[j + 1])
            fprintf(stderr, " Verify failed: \"%s\" -> \"%s\": packet %u, frame %u (status %d)\n", jobs[j]->in.c_str(),
                    jobs[j]->out.c_str(), p - p0, v.firstMismatch[p], v.status[p]);
    }
}

// --verify / --verify-source (`option`): decode the group's stream on `device` and compare it with what it was encoded from.
// batch(dec, verdict) is the library call that does both: VerifyBatch against the PCM, VerifyBatchFloat against the floats.
template <class Batch>
bool verify_encoded(const std::vector<Job *> &jobs, ALACEncoder &enc, const std::vector<uint32_t> &firstPacket, int device,
                    const char *option, Batch batch)
{
    const uint32_t np = firstPacket.back();
    if (np == 0) return true;
    uint32_t cookieSize = enc.GetMagicCookieSize(jobs[0]->info.channels);
    Bytes cookie(cookieSize, 0);
    enc.GetMagicCookie(cookie.data(), &cookieSize);
    cookie.resize(cookieSize);
    ALACDecoder dec;
    if (!open_decoder(dec, cookie, device)) {
        fprintf(stderr, " Cannot initialise the decoder for %s\n", option);
        return false;
    }
    Verdict v(np);
    if (!v.ran(batch(dec, v))) return false;
    if (v.bad) report_mismatches(jobs, firstPacket, v);
    return v.bad == 0;
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
        for (size_t j = 0; j < v.size(); j++) stage_floats(*v[j], first[j + 1] - first[j], fl.data() + (size_t)first[j] * ch);
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
            J.info.dataSize = (first[j + 1] - first[j]) * frame_bytes(J.info);
        }
    }
    return ok;
}

// --bits auto: every integer job gets the smallest depth that holds its samples exactly, found on the GPU
// (alac_hip_int_probe: one call per source depth and channel count, one segment per file), and is from then on a file of that
// depth.  A file without such a depth (a 20-bit file with bits set under its samples) is named; the run is then refused.
bool probe_int_jobs(std::vector<Job> &jobs, int device)
{
    std::map<std::pair<uint32_t, uint32_t>, std::vector<Job *> > bySource;  // (depth, channels); the container follows the depth
    for (size_t j = 0; j < jobs.size(); j++) bySource[std::make_pair(jobs[j].srcBits, jobs[j].info.channels)].push_back(&jobs[j]);
    ALACEncoder enc;
    if (device >= 0) enc.SetDevice(device);
    bool ok = true;
    for (auto g = bySource.begin(); g != bySource.end(); ++g) {
        const uint32_t ch = g->first.second, frameBytes = ch * bytes_per_sample(g->first.first);
        std::vector<Job *> &v = g->second;
        std::vector<uint64_t> first(1, 0);  // the files' frames back to back
        for (size_t j = 0; j < v.size(); j++) first.push_back(first.back() + v[j]->srcFrames);
        Bytes pcm((size_t)(first.back() * frameBytes) + 4, 0);
        for (size_t j = 0; j < v.size(); j++) stage_source(*v[j], v[j]->srcFrames, pcm.data() + (size_t)first[j] * frameBytes);
        std::vector<alac_hip_int_report> reports(v.size());
        const int32_t rc = enc.ProbeInt(pcm.data(), int_source_of(*v[0]), ch, first.back(), first.data(), (uint32_t)v.size(),
                                        reports.data());
        if (rc != ALAC_noErr) {
            fprintf(stderr, " Probing the integer input failed (status %d)\n", rc);
            return false;
        }
        for (size_t j = 0; j < v.size(); j++) {
            Job &J = *v[j];
            const alac_hip_int_report &r = reports[j];
            const uint32_t depth = alac_hip_int_report_depth(&r);
            if (depth == 0) {
                fprintf(stderr, " --bits auto: no lossless bit depth (pad_bits 0x%x, out_of_range %llu): \"%s\"\n", r.pad_bits,
                        (unsigned long long)r.out_of_range, J.in.c_str());
                ok = false;
                continue;
            }
            const bool dualMono = ch == 2 && J.srcFrames && r.differing_frames == 0;
            printf("Integer input is lossless at %u bits%s: %s\n", depth, dualMono ? ", channels identical" : "", J.in.c_str());
            J.info.bitsPerChannel = depth;
            J.info.dataSize = J.srcFrames * frame_bytes(J.info);
        }
    }
    return ok;
}

// --rate: the jobs that are to be resampled (srcRate != 0) become float jobs at o.rate: the files of one rate, channel count and
// source format go through the GPU in one call, each one segment (alac_hip_resample_int_host / _float_host).  An integer job
// holds its source as a --bits job does (srcBits, srcPos, srcFrames), a float job as a --float-bits job does.
bool resample_jobs(std::vector<Job> &jobs, const Options &o, int device)
{
    std::map<std::string, std::vector<Job *> > groups;
    for (size_t j = 0; j < jobs.size(); j++) {
        Job &J = jobs[j];
        if (!J.srcRate) continue;
        char key[64];
        snprintf(key, sizeof(key), "%u/%u/%u", J.srcRate, J.info.channels, J.srcFloat ? 0u : J.srcBits);
        groups[key].push_back(&J);
    }
    if (groups.empty()) return true;
    alac_hip_ctx *ctx = nullptr;
    const char *dev = getenv("ALAC_HIP_DEVICE");
    if (alac_hip_create(&ctx, device >= 0 ? device : (dev ? atoi(dev) : 0), nullptr) != ALAC_HIP_noErr) {
        fprintf(stderr, " Cannot create a GPU context\n");
        return false;
    }
    bool ok = true;
    for (std::map<std::string, std::vector<Job *> >::iterator g = groups.begin(); g != groups.end() && ok; ++g) {
        std::vector<Job *> &v = g->second;
        const Job &F = *v[0];
        const uint32_t ch = F.info.channels, sampleBytes = F.srcFloat ? 4u : bytes_per_sample(F.srcBits);
        std::vector<uint64_t> first(1, 0);  // the files' frames back to back
        for (size_t j = 0; j < v.size(); j++) first.push_back(first.back() + v[j]->srcFrames);
        std::vector<uint64_t> outFirst(v.size() + 1, 0);
        const uint64_t total = alac_hip_resample_frames(F.srcRate, o.rate, first.back(), first.data(), (uint32_t)v.size(), outFirst.data());
        // interleaved: channel_stride 1, frame_stride ch (room for one frame where every file is empty)
        Bytes in((size_t)(first.back() * ch * sampleBytes) + 4 * ch, 0);
        for (size_t j = 0; j < v.size(); j++) {
            uint8_t *dst = in.data() + (size_t)(first[j] * ch * sampleBytes);
            if (F.srcFloat) {
                const uint64_t bytes = v[j]->srcFrames * ch * 4;
                memcpy(dst, v[j]->file.data() + v[j]->floatPos, (size_t)bytes);
                if (v[j]->floatBigEndian) alacfile::swap_samples_in_place(dst, bytes, 32);
            } else {
                stage_source(*v[j], v[j]->srcFrames, dst);
            }
        }
        std::vector<float> rows((size_t)(total * ch) + 1, 0.0f);
        std::vector<alac_hip_resample_report> reports(v.size());
        int32_t rc;
        if (F.srcFloat) {
            rc = alac_hip_resample_float_host(ctx, (const float *)in.data(), ch, 1, ch, F.srcRate, o.rate, first.back(), first.data(),
                                              (uint32_t)v.size(), rows.data(), total, total, reports.data());
        } else {
            const alac_hip_int_source src = int_source_of(F);
            rc = alac_hip_resample_int_host(ctx, in.data(), &src, ch, F.srcRate, o.rate, first.back(), first.data(),
                                            (uint32_t)v.size(), rows.data(), total, total, reports.data());
        }
        if (rc != ALAC_HIP_noErr) {
            fprintf(stderr, " Resampling to %u Hz failed (status %d: %s)\n", o.rate, rc, alac_hip_last_error(ctx));
            ok = false;
            break;
        }
        for (size_t j = 0; j < v.size(); j++) {
            Job &J = *v[j];
            const uint64_t n = reports[j].out_frames;
            J.resampled.assign((size_t)(n * ch) + 1, 0.0f);
            for (uint32_t c = 0; c < ch; c++) {
                const float *row = rows.data() + (size_t)(c * total + reports[j].out_first);
                for (uint64_t i = 0; i < n; i++) J.resampled[(size_t)(i * ch + c)] = row[i];
            }
            if (reports[j].nonfinite)
                fprintf(stderr, " Warning: %llu non-finite samples read as 0: \"%s\"\n", (unsigned long long)reports[j].nonfinite,
                        J.in.c_str());
            if (reports[j].peak > 1.0)
                fprintf(stderr, " Warning: the peak after resampling is %.2f dBFS, above full scale: \"%s\"\n",
                        20.0 * log10(reports[j].peak), J.in.c_str());
            J.info.sampleRate = o.rate;
            J.info.dataSize = n * frame_bytes(J.info);
        }
    }
    alac_hip_destroy(ctx);
    return ok;
}

// ---- encode: all jobs share bit depth and channel count; each file is one segment ----
bool encode_group(std::vector<Job *> &jobs, const Options &o, int device)
{
    const InputInfo &first = jobs[0]->info;
    const uint32_t ch = first.channels, bytesPerFrame = (uint32_t)frame_bytes(first), frame = kALACDefaultFramesPerPacket;
    const uint64_t packetBytes = (uint64_t)bytesPerFrame * frame;

    ALACEncoder enc;
    enc.SetFrameSize(frame);
    enc.SetLPCMode(o.lpc);
    if (o.dither.on) enc.SetDither(ALAC_HIP_DITHER_TPDF, o.dither.seed);
    if (device >= 0) enc.SetDevice(device);
    AudioFormatDescription outFmt = alac_format(first);
    if (enc.InitializeEncoder(outFmt, 0) != ALAC_noErr) {
        fprintf(stderr, " Cannot initialise the encoder (status %d)\n", enc.LastStatus());
        return false;
    }

    // packets back to back at the full-packet stride
    std::vector<uint64_t> dataBytes;
    for (size_t j = 0; j < jobs.size(); j++) dataBytes.push_back(jobs[j]->info.dataSize);
    const plan::PacketCut cut = plan::cut_packets(dataBytes, bytesPerFrame, frame, o.segmentPackets);
    const std::vector<uint32_t> &numSamples = cut.numSamples, &firstPacket = cut.firstPacket, &segs = cut.segments;
    const uint32_t np = (uint32_t)numSamples.size();

    Bytes stream((size_t)np * (packetBytes + kALACMaxEscapeHeaderBytes));
    std::vector<uint32_t> sizes(np, 0);
    uint64_t total = 0;
    auto encoded = [](int32_t rc) {
        if (rc != ALAC_noErr) fprintf(stderr, " Encoding failed (status %d)\n", rc);
        return rc == ALAC_noErr;
    };
    if (np && jobs[0]->floatIn) {
        // interleaved floats at the full-packet stride: channel_stride 1, frame_stride ch
        std::vector<float> fl((size_t)np * frame * ch, 0.0f);
        std::vector<uint32_t> clipped(np, 0);
        // every file's frames count from 0: its dither does not depend on the files beside it
        std::vector<uint64_t> origin(np, 0);
        for (size_t j = 0; j < jobs.size(); j++) {
            stage_floats(*jobs[j], jobs[j]->info.dataSize / bytesPerFrame, fl.data() + (size_t)firstPacket[j] * frame * ch);
            for (uint32_t p = firstPacket[j]; p < firstPacket[j + 1]; p++) origin[p] = (uint64_t)(p - firstPacket[j]) * frame;
        }
        if (!encoded(enc.EncodeSegmentsFloatAt(fl.data(), 1, ch, numSamples.data(), np, segs.data(), (uint32_t)segs.size() - 1,
                                               stream.data(), stream.size(), sizes.data(), &total, clipped.data(), origin.data())))
            return false;
        for (size_t j = 0; j < jobs.size(); j++) {
            uint64_t clips = 0;
            for (uint32_t p = firstPacket[j]; p < firstPacket[j + 1]; p++) clips += clipped[p];
            if (clips)
                fprintf(stderr, " Warning: %llu samples clipped to %u bits: \"%s\"\n", (unsigned long long)clips,
                        first.bitsPerChannel, jobs[j]->in.c_str());
        }
        if (o.verifySource &&
            !verify_encoded(jobs, enc, firstPacket, device, "--verify-source", [&](ALACDecoder &dec, Verdict &v) {
                return dec.VerifyBatchFloat(stream.data(), sizes.data(), np, fl.data(), 1, ch, numSamples.data(),
                                            o.dither.on ? ALAC_HIP_DITHER_TPDF : ALAC_HIP_DITHER_NONE, o.dither.seed, origin.data(),
                                            v.firstMismatch.data(), v.status.data(), &v.bad);
            }))
            return false;
    } else if (np) {
        Bytes pcm((size_t)np * packetBytes, 0);
        for (size_t j = 0; j < jobs.size(); j++) {
            const Job &J = *jobs[j];
            uint8_t *dst = pcm.data() + (size_t)firstPacket[j] * packetBytes;
            const uint32_t mine = firstPacket[j + 1] - firstPacket[j];
            if (J.intConv && mine) {
                // --bits: the file's own containers through the integer rule into its packets; its frames count from 0
                Bytes src((size_t)(J.srcFrames * ch * bytes_per_sample(J.srcBits)));
                stage_source(J, J.srcFrames, src.data());
                std::vector<uint32_t> clipped(mine, 0);
                const int32_t rc = enc.RequantizeInt(src.data(), int_source_of(J), ch, first.bitsPerChannel, frame,
                                                     numSamples.data() + firstPacket[j], mine, dst, (uint64_t)mine * packetBytes,
                                                     clipped.data(), o.dither.on ? ALAC_HIP_DITHER_TPDF : ALAC_HIP_DITHER_NONE,
                                                     o.dither.seed);
                if (rc != ALAC_noErr) {
                    fprintf(stderr, " Converting to %u bits failed (status %d): \"%s\"\n", first.bitsPerChannel, rc, J.in.c_str());
                    return false;
                }
                uint64_t clips = 0;
                for (uint32_t p = 0; p < mine; p++) clips += clipped[p];
                if (clips)
                    fprintf(stderr, " Warning: %llu samples clipped to %u bits: \"%s\"\n", (unsigned long long)clips,
                            first.bitsPerChannel, J.in.c_str());
            } else if (!J.intConv) {
                memcpy(dst, J.file.data() + J.info.dataPos, (size_t)J.info.dataSize);
                if (J.info.bigEndianPcm) alacfile::swap_samples_in_place(dst, J.info.dataSize, J.info.bitsPerChannel);
            }
        }
        if (!encoded(enc.EncodeSegments(pcm.data(), numSamples.data(), np, segs.data(), (uint32_t)segs.size() - 1, stream.data(),
                                        stream.size(), sizes.data(), &total)))
            return false;
        if (o.verify &&
            !verify_encoded(jobs, enc, firstPacket, device, "--verify", [&](ALACDecoder &dec, Verdict &v) {
                return dec.VerifyBatch(stream.data(), sizes.data(), np, pcm.data(), numSamples.data(), v.firstMismatch.data(),
                                       v.status.data(), &v.bad);
            }))
            return false;
    }
    // per file: cookie + container
    std::vector<uint64_t> offs(np + 1, 0);
    for (uint32_t p = 0; p < np; p++) offs[p + 1] = offs[p] + sizes[p];
    for (size_t j = 0; j < jobs.size(); j++) {
        Job &J = *jobs[j];
        // the cookie carries the file's own sample rate; no packet size or bit rate in it, as a fresh encoder reports it
        const alac_hip_format fmt = {frame, J.info.bitsPerChannel, J.info.channels, (uint32_t)J.info.sampleRate};
        Bytes cookie(alac_hip_magic_cookie_size(&fmt), 0);
        cookie.resize(alac_hip_magic_cookie_full(&fmt, 0, 0, cookie.data(), (uint32_t)cookie.size()));
        const uint32_t p0 = firstPacket[j], p1 = firstPacket[j + 1];
        const std::vector<uint32_t> mine(sizes.begin() + p0, sizes.begin() + p1);
        if (alacfile::has_m4a_extension(J.out)) {
            const alacfile::AlacM4aParams mp = {(uint32_t)J.info.sampleRate, J.info.channels, J.info.bitsPerChannel, frame,
                                                J.info.dataSize / bytesPerFrame};
            J.result = alacfile::build_alac_m4a(mp, cookie, mine, stream.data() + offs[p0], offs[p1] - offs[p0]);
        } else {
            const alacfile::AlacCafParams cp = {J.info.sampleRate, J.info.channels, J.info.bitsPerChannel, frame, J.info.dataSize};
            J.result = alacfile::build_alac_caf(cp, cookie, mine, stream.data() + offs[p0], offs[p1] - offs[p0]);
        }
    }
    return true;
}

// ---- --compare <alac file> <reference pcm file>: decode and compare on the GPU, write nothing; 0 = identical ----
int compare_files(const Options &o)
{
    Job A, R;
    A.in = o.files[0];
    R.in = o.files[1];
    for (Job *J : {&A, &R})  // the reference may be float PCM
        if (!read_job(*J) || refused(alacfile::sniff_input(J->file, J->info, J == &R), *J)) return 1;
    const bool floatRef = !R.info.isAlac && R.info.isFloat;
    if (floatRef && R.info.bitsPerChannel != 32) {
        fprintf(stderr, " %u-bit float reference is not supported (32-bit float): \"%s\"\n", R.info.bitsPerChannel, R.in.c_str());
        return 1;
    }
    if (o.dither.on && !floatRef) {
        fprintf(stderr, " --compare --dither needs a 32-bit float reference: \"%s\"\n", R.in.c_str());
        return 1;
    }
    if (!A.info.isAlac || R.info.isAlac) {
        fprintf(stderr, " --compare takes an ALAC file (CAF or M4A) and a PCM reference (WAV or CAF)\n");
        return 1;
    }
    if (refused(parse_alac(A), A)) return 1;
    ALACDecoder dec;
    if (!open_decoder(dec, A.contents.cookie, -1)) {
        fprintf(stderr, " Cannot initialise the decoder from the magic cookie\n");
        return 1;
    }
    const uint32_t ch = dec.mConfig.numChannels, bits = dec.mConfig.bitDepth, frame = dec.mConfig.frameLength;
    if (o.dither.on && bits == 32) {
        fprintf(stderr, " --dither needs a 16-, 20- or 24-bit stream: \"%s\"\n", A.in.c_str());
        return 1;
    }
    if (ch != R.info.channels || (!floatRef && bits != R.info.bitsPerChannel)) {
        printf("Compare: \"%s\" is %u-bit %u-channel, \"%s\" %u-bit %u-channel: different\n", A.in.c_str(), bits, ch,
               R.in.c_str(), R.info.bitsPerChannel, R.info.channels);
        return 1;
    }
    // bytes of one frame of the reference: float32 samples, or the stream's own integer containers
    const uint64_t bytesPerFrame = (uint64_t)ch * (floatRef ? 4 : bytes_per_sample(bits)), packetBytes = bytesPerFrame * frame;
    std::vector<uint32_t> sizes;
    Bytes stream;
    append_packets(A, stream, sizes);
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
    Verdict v(np);
    if (np && !v.ran(floatRef ? dec.VerifyBatchFloat(stream.data(), sizes.data(), np, (const float *)pcm.data(), 1, ch, expected.data(),
                                                     o.dither.on ? ALAC_HIP_DITHER_TPDF : ALAC_HIP_DITHER_NONE, o.dither.seed,
                                                     nullptr, v.firstMismatch.data(), v.status.data(), &v.bad)
                              : dec.VerifyBatch(stream.data(), sizes.data(), np, pcm.data(), expected.data(),
                                                v.firstMismatch.data(), v.status.data(), &v.bad)))
        return 1;
    const uint32_t p = v.bad ? v.first_bad(0, np) : np;
    if (p < np) {
        printf("Compare: \"%s\" differs from \"%s\" at packet %u, frame %u (sample-frame %llu, status %d)\n", A.in.c_str(),
               R.in.c_str(), p, v.firstMismatch[p], (unsigned long long)((uint64_t)p * frame + v.firstMismatch[p]), v.status[p]);
        return 1;
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
bool decode_group(std::vector<Job *> &jobs, int device)
{
    ALACDecoder dec;
    if (!open_decoder(dec, jobs[0]->contents.cookie, device)) {
        fprintf(stderr, " Cannot initialise the decoder from the magic cookie\n");
        return false;
    }
    const uint32_t ch = dec.mConfig.numChannels, bits = dec.mConfig.bitDepth, frame = dec.mConfig.frameLength;
    for (size_t j = 0; j < jobs.size(); j++)
        if (!cookie_matches_description(bits, *jobs[j])) return false;
    const uint32_t bytesPerFrame = ch * bytes_per_sample(bits);
    std::vector<uint32_t> sizes;
    Bytes stream;
    const std::vector<uint32_t> firstPacket = gather_packets(jobs, stream, sizes);
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
        Bytes outPcm;
        for (uint32_t p = firstPacket[j]; p < firstPacket[j + 1]; p++) {
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

// ---- --devices N ----
bool devices_ok(uint32_t devices)
{
    if (!devices) return true;
    const int32_t have = alac_hip_device_count();
    // ALACCONVERT_SHARE_DEVICES=1 (tests on a one-GPU box): the N workers run side by side on the devices there are
    if (have < 1 || ((int32_t)devices > have && !getenv("ALACCONVERT_SHARE_DEVICES"))) {
        fprintf(stderr, " --devices %u: only %d GPU(s) visible\n", devices, have);
        return false;
    }
    return true;
}

// The files of every group dealt to the workers (plan::deal): one host thread and one context per device, every Job with one
// worker.  fn(jobs, device) runs on what one worker takes of one group; a worker stops at the first false, which is then
// the answer.  Without --devices: one worker, device -1 (the classes' default, ALAC_HIP_DEVICE or 0).
template <class F>
bool run_dealt(const Groups &groups, uint32_t devices, F fn)
{
    std::vector<const std::vector<Job *> *> group;
    std::vector<size_t> groupSizes;
    for (Groups::const_iterator g = groups.begin(); g != groups.end(); ++g) {
        group.push_back(&g->second);
        groupSizes.push_back(g->second.size());
    }
    const uint32_t workers = devices ? devices : 1;
    const int32_t visible = devices ? alac_hip_device_count() : 1;
    const std::vector<std::vector<plan::Part> > perWorker = plan::deal(groupSizes, workers);
    std::vector<int> ok(workers, 1);
    plan::run_workers(workers, [&](uint32_t k) {
        for (size_t i = 0; i < perWorker[k].size() && ok[k]; i++) {
            std::vector<Job *> jobs;
            for (size_t m : perWorker[k][i].members) jobs.push_back((*group[perWorker[k][i].group])[m]);
            ok[k] = fn(jobs, devices ? (int)(k % (uint32_t)visible) : -1);
        }
    });
    for (uint32_t k = 0; k < workers; k++)
        if (!ok[k]) return false;
    return true;
}

// ---- --crc / --crc-check: the CRC-32 of every file's PCM, computed on the GPU; nothing is written ----
// ALAC files of one cookie: one TestBatch, one range per file
void crc_alac_group(std::vector<Job *> &jobs, int device)
{
    ALACDecoder dec;
    if (!open_decoder(dec, jobs[0]->contents.cookie, device)) {
        fprintf(stderr, " Cannot initialise the decoder from the magic cookie: \"%s\"\n", jobs[0]->in.c_str());
        return;
    }
    const uint32_t bits = dec.mConfig.bitDepth, bytesPerFrame = dec.mConfig.numChannels * bytes_per_sample(bits);
    std::vector<Job *> take;
    for (size_t j = 0; j < jobs.size(); j++)
        if (cookie_matches_description(bits, *jobs[j])) take.push_back(jobs[j]);
    if (take.empty()) return;
    std::vector<uint32_t> sizes;
    Bytes stream;
    const std::vector<uint32_t> firstPacket = gather_packets(take, stream, sizes);
    const uint32_t np = (uint32_t)sizes.size();
    std::vector<alac_hip_pcm_digest> digests(take.size());
    std::vector<uint32_t> frames(np, 0);
    std::vector<int32_t> status(np, 0);
    const int32_t rc = dec.TestBatch(stream.data(), sizes.data(), np, firstPacket.data(), (uint32_t)take.size(), digests.data(),
                                     frames.data(), status.data());
    if (rc != ALAC_noErr) {
        fprintf(stderr, " Decoding failed (status %d): \"%s\"\n", rc, take[0]->in.c_str());
        return;
    }
    for (size_t j = 0; j < take.size(); j++) {
        Job &J = *take[j];
        uint32_t p = firstPacket[j];
        while (p < firstPacket[j + 1] && status[p] == 0) p++;
        if (p < firstPacket[j + 1]) {
            fprintf(stderr, " Cannot decode packet %u (status %d): \"%s\"\n", p - firstPacket[j], status[p], J.in.c_str());
            continue;
        }
        J.crc = digests[j].crc32;
        J.crcFrames = digests[j].bytes / bytesPerFrame;
        J.done = true;
    }
}

// integer PCM files: the sample bytes of all of them staged in one buffer, one range per file
void crc_pcm_group(std::vector<Job *> &jobs, int device)
{
    std::vector<uint64_t> ranges;
    Bytes pcm;
    for (size_t j = 0; j < jobs.size(); j++) {
        const InputInfo &in = jobs[j]->info;
        // whole frames only: the encoder drops a trailing fraction of a frame (ALACEncoder.cu:984)
        const uint64_t bytes = in.dataSize / frame_bytes(in) * frame_bytes(in);
        ranges.push_back(pcm.size()), ranges.push_back(bytes);
        jobs[j]->crcFrames = bytes / frame_bytes(in);
        pcm.insert(pcm.end(), jobs[j]->file.begin() + in.dataPos, jobs[j]->file.begin() + in.dataPos + bytes);
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
void crc_run(std::vector<Job> &jobs, uint32_t devices)
{
    Groups groups;  // ALAC files by cookie ("D..."), all PCM files ("P")
    for (size_t j = 0; j < jobs.size(); j++) {
        Job &J = jobs[j];
        if (!read_job(J)) continue;
        J.opened = true;
        std::string err = alacfile::sniff_input(J.file, J.info, true);
        if (err.empty() && J.info.isAlac) err = parse_alac(J);
        if (refused(err, J)) continue;
        if (!J.info.isAlac && J.info.isFloat) {
            fprintf(stderr, " --crc does not take float PCM: \"%s\"\n", J.in.c_str());
            continue;
        }
        if (!J.info.isAlac && !pcm_format_ok(J)) continue;
        groups[J.info.isAlac ? cookie_key(J) : std::string("P")].push_back(&J);
    }
    run_dealt(groups, devices, [](std::vector<Job *> &part, int device) {
        (part[0]->info.isAlac ? crc_alac_group : crc_pcm_group)(part, device);
        return true;
    });
}

int crc_files(const Options &o)
{
    if (!devices_ok(o.devices)) return 1;
    std::vector<Job> jobs(o.files.size());
    for (size_t j = 0; j < jobs.size(); j++) jobs[j].in = o.files[j];
    crc_run(jobs, o.devices);
    int rc = 0;
    for (size_t j = 0; j < jobs.size(); j++) {
        if (jobs[j].done) printf("%08x  %llu  %s\n", jobs[j].crc, (unsigned long long)jobs[j].crcFrames, jobs[j].in.c_str());
        else rc = 1;
    }
    return rc;
}

int crc_check(const Options &o)
{
    if (!devices_ok(o.devices)) return 1;
    std::ifstream list(o.crcList.c_str());
    if (!list) {
        fprintf(stderr, " Cannot open file \"%s\"\n", o.crcList.c_str());
        return 1;
    }
    std::vector<Job> jobs;
    std::vector<uint32_t> wantCrc;
    std::vector<uint64_t> wantFrames;
    int rc = 0;
    std::string line;
    for (unsigned n = 1; std::getline(list, line); n++) {
        if (line.empty()) continue;
        Job J;
        uint32_t crc = 0;
        uint64_t frames = 0;
        if (!plan::parse_crc_line(line, crc, frames, J.in)) {
            fprintf(stderr, " %s: line %u is not \"<crc32>  <frames>  <path>\"\n", o.crcList.c_str(), n);
            rc = 1;
            continue;
        }
        jobs.push_back(J);
        wantCrc.push_back(crc);
        wantFrames.push_back(frames);
    }
    crc_run(jobs, o.devices);
    for (size_t j = 0; j < jobs.size(); j++) {
        const bool ok = jobs[j].done && jobs[j].crc == wantCrc[j] && jobs[j].crcFrames == wantFrames[j];
        printf("%s: %s\n", jobs[j].in.c_str(), ok ? "OK" : jobs[j].opened ? "FAILED" : "FAILED open");
        if (!ok) rc = 1;
    }
    return rc;
}

// ---- --loudness: integrated loudness and sample peak of every file, measured on the GPU; nothing is written ----
// ALAC files of one cookie: one LoudnessBatch (truePeak: one LoudnessTruePeakBatch), one segment per file
void loudness_alac_group(std::vector<Job *> &jobs, int device, bool truePeak)
{
    ALACDecoder dec;
    if (!open_decoder(dec, jobs[0]->contents.cookie, device)) {
        fprintf(stderr, " Cannot initialise the decoder from the magic cookie: \"%s\"\n", jobs[0]->in.c_str());
        return;
    }
    std::vector<Job *> take;
    for (size_t j = 0; j < jobs.size(); j++)
        if (cookie_matches_description(dec.mConfig.bitDepth, *jobs[j])) take.push_back(jobs[j]);
    if (take.empty()) return;
    std::vector<uint32_t> sizes;
    Bytes stream;
    const std::vector<uint32_t> firstPacket = gather_packets(take, stream, sizes);
    const uint32_t np = (uint32_t)sizes.size();
    std::vector<double> lufs(take.size()), peak(take.size()), tp(take.size(), 0.0);
    std::vector<uint32_t> frames(np, 0);
    std::vector<int32_t> status(np, 0);
    const int32_t rc = truePeak ? dec.LoudnessTruePeakBatch(stream.data(), sizes.data(), np, firstPacket.data(), (uint32_t)take.size(),
                                                            lufs.data(), peak.data(), tp.data(), frames.data(), status.data())
                                : dec.LoudnessBatch(stream.data(), sizes.data(), np, firstPacket.data(), (uint32_t)take.size(),
                                                    lufs.data(), peak.data(), frames.data(), status.data());
    if (rc != ALAC_noErr) {
        fprintf(stderr, " Measuring failed (status %d): \"%s\"\n", rc, take[0]->in.c_str());
        return;
    }
    for (size_t j = 0; j < take.size(); j++) {
        Job &J = *take[j];
        uint32_t p = firstPacket[j];
        while (p < firstPacket[j + 1] && status[p] == 0) p++;
        if (p < firstPacket[j + 1]) {
            fprintf(stderr, " Cannot decode packet %u (status %d): \"%s\"\n", p - firstPacket[j], status[p], J.in.c_str());
            continue;
        }
        J.crcFrames = 0;
        for (p = firstPacket[j]; p < firstPacket[j + 1]; p++) J.crcFrames += frames[p];
        J.lufs = lufs[j], J.peak = peak[j], J.truePeak = tp[j];
        J.done = true;
    }
}

// PCM files, integer or float: each one staged and measured as one segment
void loudness_pcm_group(std::vector<Job *> &jobs, int device, bool truePeak)
{
    alac_hip_ctx *ctx = nullptr;
    const char *dev = getenv("ALAC_HIP_DEVICE");
    if (alac_hip_create(&ctx, device >= 0 ? device : (dev ? atoi(dev) : 0), nullptr) != ALAC_HIP_noErr) {
        fprintf(stderr, " Cannot create a GPU context\n");
        return;
    }
    for (size_t j = 0; j < jobs.size(); j++) {
        Job &J = *jobs[j];
        const InputInfo &in = J.info;
        const uint32_t C = in.channels, rate = (uint32_t)in.sampleRate;
        // whole frames only: the encoder drops a trailing fraction of a frame (ALACEncoder.cu:984)
        const uint64_t frames = in.dataSize / frame_bytes(in), bytes = frames * frame_bytes(in);
        Bytes pcm(J.file.begin() + in.dataPos, J.file.begin() + in.dataPos + bytes);
        if (in.bigEndianPcm) alacfile::swap_samples_in_place(pcm.data(), bytes, in.bitsPerChannel);
        const uint64_t rows = (double)rate == in.sampleRate ? alac_hip_loudness_rows(rate, frames, nullptr, 1) : 0;
        std::vector<double> energy((size_t)rows * C + 1);
        alac_hip_loudness_report rep = {};
        int32_t rc = ALAC_HIP_ParamError;
        if ((double)rate != in.sampleRate) {
            // (a fractional rate: refused like every other rate that is not a multiple of 10)
        } else if (in.isFloat) {
            rc = alac_hip_loudness_float_host(ctx, (const float *)pcm.data(), C, 1, C, rate, frames, nullptr, 1, energy.data(), rows,
                                              &rep);
        } else {
            const alac_hip_int_source src = {bytes_per_sample(in.bitsPerChannel), in.bitsPerChannel, 1, 0, 1, C};
            rc = alac_hip_loudness_int_host(ctx, pcm.data(), &src, C, rate, frames, nullptr, 1, energy.data(), rows, &rep);
        }
        if (rc == ALAC_HIP_noErr) rc = alac_hip_loudness_integrated(energy.data(), rep.num_blocks, C, rate / 10, nullptr, &J.lufs);
        if (rc == ALAC_HIP_noErr && truePeak) {
            double channelPeak[8];
            alac_hip_true_peak_report tp = {};
            if (in.isFloat) {
                rc = alac_hip_true_peak_float_host(ctx, (const float *)pcm.data(), C, 1, C, rate, frames, nullptr, 1, channelPeak, &tp);
            } else {
                const alac_hip_int_source src = {bytes_per_sample(in.bitsPerChannel), in.bitsPerChannel, 1, 0, 1, C};
                rc = alac_hip_true_peak_int_host(ctx, pcm.data(), &src, C, rate, frames, nullptr, 1, channelPeak, &tp);
            }
            J.truePeak = tp.true_peak;
        }
        if (rc != ALAC_HIP_noErr) {
            fprintf(stderr, " Measuring failed (status %d): %s: \"%s\"\n", rc, alac_hip_last_error(ctx), J.in.c_str());
            continue;
        }
        J.peak = rep.peak;
        J.crcFrames = frames;
        J.done = true;
    }
    alac_hip_destroy(ctx);
}

int loudness_files(const Options &o)
{
    if (!devices_ok(o.devices)) return 1;
    std::vector<Job> jobs(o.files.size());
    Groups groups;  // ALAC files by cookie ("D..."), all PCM files ("P")
    for (size_t j = 0; j < jobs.size(); j++) {
        Job &J = jobs[j];
        J.in = o.files[j];
        if (!read_job(J)) continue;
        std::string err = alacfile::sniff_input(J.file, J.info, true);
        if (err.empty() && J.info.isAlac) err = parse_alac(J);
        if (refused(err, J)) continue;
        if (!J.info.isAlac && J.info.isFloat && (J.info.bitsPerChannel != 32 || J.info.channels < 1 || J.info.channels > 8)) {
            fprintf(stderr, " %u-bit %u-channel float input is not supported (32-bit float, 1 to 8 channels): \"%s\"\n",
                    J.info.bitsPerChannel, J.info.channels, J.in.c_str());
            continue;
        }
        if (!J.info.isAlac && !J.info.isFloat && !pcm_format_ok(J)) continue;
        groups[J.info.isAlac ? cookie_key(J) : std::string("P")].push_back(&J);
    }
    run_dealt(groups, o.devices, [&](std::vector<Job *> &part, int device) {
        (part[0]->info.isAlac ? loudness_alac_group : loudness_pcm_group)(part, device, o.truePeak);
        return true;
    });
    int rc = 0;
    for (size_t j = 0; j < jobs.size(); j++) {
        const Job &J = jobs[j];
        if (!J.done) {
            rc = 1;
            continue;
        }
        // printf writes -inf for the logarithm of nothing: a silent file has neither a loudness nor a peak in dB
        if (o.truePeak)
            printf("%.2f LUFS  %.2f dBFS  %.2f dBTP  %llu  %s\n", J.lufs, 20.0 * log10(J.peak), 20.0 * log10(J.truePeak),
                   (unsigned long long)J.crcFrames, J.in.c_str());
        else
            printf("%.2f LUFS  %.2f dBFS  %llu  %s\n", J.lufs, 20.0 * log10(J.peak), (unsigned long long)J.crcFrames, J.in.c_str());
    }
    return rc;
}

// ---- the conversions: <in> <out> pairs, PCM in -> ALAC out, ALAC in -> PCM out ----
int convert(const Options &o)
{
    // every file opened and sniffed, in the order of the command line
    std::vector<Job> jobs(o.files.size() / 2);
    for (size_t j = 0; j < jobs.size(); j++) {
        Job &J = jobs[j];
        J.in = o.files[2 * j];
        J.out = o.files[2 * j + 1];
        if (!read_job(J)) return 1;
        printf("Input file: %s\n", J.in.c_str());
        printf("Output file: %s\n", J.out.c_str());
        if (refused(alacfile::sniff_input(J.file, J.info, o.floatInput() || o.intConvert() || o.rate), J)) return 1;
        if (o.rate && J.info.isAlac) {  // --rate is encode only
            plan::usage();
            return 1;
        }
        if (o.rate && J.info.sampleRate == (double)o.rate) {
            fprintf(stderr, " Already at %u Hz, not resampled: \"%s\"\n", o.rate, J.in.c_str());
        } else if (o.rate) {
            uint32_t L = 0, M = 0, K = 0;
            const uint32_t srcRate = (uint32_t)J.info.sampleRate;
            if ((double)srcRate != J.info.sampleRate || alac_hip_resample_filter(srcRate, o.rate, &L, &M, &K, nullptr) != ALAC_HIP_noErr) {
                plan::usage();
                return 1;
            }
            if (J.info.isFloat && !o.floatBits) {
                fprintf(stderr, " --rate with float PCM input needs --float-bits N: \"%s\"\n", J.in.c_str());
                return 1;
            }
            if (J.info.isFloat ? J.info.bitsPerChannel != 32 : !plan::pcm_depth_ok(J.info.bitsPerChannel)) {
                fprintf(stderr, " File \"%s\'s\" data format is of an unsupported type\n", J.in.c_str());
                return 1;
            }
            if (J.info.channels < 1 || J.info.channels > 8) {
                fprintf(stderr, " File \"%s\'s\" data format is of an unsupported type\n", J.in.c_str());
                return 1;
            }
            // from here on the file is the integer file of its resampled, quantized samples (resample_jobs below fills in the
            // frames); the source stays where it is
            J.srcRate = srcRate;
            J.srcFloat = J.info.isFloat;
            J.srcBits = J.info.bitsPerChannel;
            J.srcPos = J.floatPos = J.info.dataPos;
            J.srcBigEndian = J.floatBigEndian = J.info.bigEndianPcm;
            J.srcFrames = J.info.dataSize / ((uint64_t)J.info.channels * bytes_per_sample(J.info.bitsPerChannel));
            J.floatIn = true;
            J.info.isFloat = J.info.bigEndianPcm = false;
            if (o.floatBits) J.info.bitsPerChannel = o.floatBits;
            J.info.dataSize = 0;
            continue;
        }
        if (o.floatInput()) {
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
            J.info.bitsPerChannel = o.floatAuto ? 32 : o.floatBits;
            J.info.dataSize = frames * frame_bytes(J.info);
        }
        if (!J.info.isAlac && !pcm_format_ok(J)) return 1;
        if (o.intConvert()) {
            if (J.info.isAlac || J.info.isFloat) {
                fprintf(stderr, " --bits takes integer PCM input, not float PCM or ALAC: \"%s\"\n", J.in.c_str());
                return 1;
            }
            if (o.dither.on && o.intBits >= J.info.bitsPerChannel) {
                fprintf(stderr, " --dither with --bits %u would round nothing in a %u-bit file: \"%s\"\n", o.intBits,
                        J.info.bitsPerChannel, J.in.c_str());
                return 1;
            }
            // from here on the file is the integer file of its converted samples; the containers stay where they are
            J.intConv = true;
            J.srcBits = J.info.bitsPerChannel;
            J.srcPos = J.info.dataPos;
            J.srcBigEndian = J.info.bigEndianPcm;
            J.srcFrames = J.info.dataSize / frame_bytes(J.info);
            J.info.bigEndianPcm = false;
            // (auto: the file's own depth until probe_int_jobs below has its lossless one)
            if (!o.intAuto) J.info.bitsPerChannel = o.intBits;
            J.info.dataSize = J.srcFrames * frame_bytes(J.info);
        }
    }
    if (o.floatAuto && !probe_float_jobs(jobs, o.devices ? 0 : -1)) return 1;
    if (o.intAuto && !probe_int_jobs(jobs, o.devices ? 0 : -1)) return 1;
    if (o.rate && !resample_jobs(jobs, o, o.devices ? 0 : -1)) return 1;

    // group: encode jobs by (depth, channels); decode jobs by cookie
    Groups groups;
    for (size_t j = 0; j < jobs.size(); j++) {
        Job &J = jobs[j];
        if (J.info.isAlac && refused(parse_alac(J), J)) return 1;
        char key[64];
        // (with --rate a run can hold float jobs, the resampled files, next to integer ones, the files already at that rate)
        snprintf(key, sizeof(key), "E%u/%u%s", J.info.bitsPerChannel, J.info.channels, J.floatIn ? "f" : "");
        groups[J.info.isAlac ? cookie_key(J) : std::string(key)].push_back(&J);
    }
    if (!devices_ok(o.devices)) return 1;
    if (!run_dealt(groups, o.devices, [&](std::vector<Job *> &part, int device) {
            return part[0]->info.isAlac ? decode_group(part, device) : encode_group(part, o, device);
        }))
        return 1;
    for (size_t j = 0; j < jobs.size(); j++) {
        if (!alacfile::write_file(jobs[j].out, jobs[j].result)) {
            fprintf(stderr, " Cannot open file \"%s\"\n", jobs[j].out.c_str());
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char *argv[])
{
    Options o;
    if (!plan::parse_args(argc, argv, o)) return 1;
    if (o.loudness) return loudness_files(o);
    if (o.crc) return crc_files(o);
    if (!o.crcList.empty()) return crc_check(o);
    return o.compare ? compare_files(o) : convert(o);
}
