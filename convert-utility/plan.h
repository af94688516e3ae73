/*
 * plan.h — the parts of alacconvert that are pure: what the command line asks for, how a group of files is cut into
 * packets and segments, which worker takes which file, one line of a --crc list.  Plain host C++17: no GPU, no library, no
 * files; parse_args and usage print.  tests/cpp/convert_plan.cpp runs every piece on its own.
 */
#ifndef ALACCONVERT_PLAN_H
#define ALACCONVERT_PLAN_H

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

namespace plan {

inline bool pcm_depth_ok(uint32_t bits) { return bits == 16 || bits == 20 || bits == 24 || bits == 32; }
inline uint32_t bytes_per_sample(uint32_t bits) { return (bits + 7) >> 3; }  // 20 bits: 3-byte containers (container.cpp)

// --dither: TPDF dither with this seed on the float inputs
struct DitherOption {
    bool on = false;
    uint64_t seed = 0;
};

struct Options {
    std::vector<std::string> files;
    bool batch = false, lpc = false, verify = false, verifySource = false, compare = false, crc = false;
    bool loudness = false;  // --loudness: no other option but --devices N and --true-peak
    bool truePeak = false;  // --true-peak: only with --loudness
    std::string crcList;  // --crc-check <list>
    uint32_t segmentPackets = 0, devices = 0, floatBits = 0;
    bool floatAuto = false;  // --float-bits auto: floatBits stays 0, every file gets its own depth from the probe
    DitherOption dither;
    bool floatInput() const { return floatBits != 0 || floatAuto; }
    // --bits N / --bits auto: integer PCM inputs are converted to N bits (auto: every file to its own lossless depth, intBits
    // stays 0) in front of the encode; bitsNamed: the command line names --bits, whatever came of it
    uint32_t intBits = 0;
    bool intAuto = false, bitsNamed = false;
    bool intConvert() const { return intBits != 0 || intAuto; }
    // --rate R: integer and float PCM inputs are resampled to R Hz on the GPU in front of the encode (0: not given)
    uint32_t rate = 0;
};

inline void usage()
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

// the lines of --bits, printed behind usage() where the command line names --bits (usage() itself prints what it always has)
inline void usage_bits()
{
    printf("        alacconvert --bits N [--dither [--dither-seed S]] [--batch] [--lpc] [--verify] ... <input wav or caf file> <output caf or m4a file> ...\n");
    printf("            (integer PCM inputs converted to N = 16, 20, 24 or 32 bits on the GPU by the integer rule: widened exactly, or\n");
    printf("             reduced with round half to even and, with --dither, TPDF dither; --verify checks against the converted PCM)\n");
    printf("        alacconvert --bits auto [--batch] [--lpc] [--verify] ... <input wav or caf file> <output caf or m4a file> ...\n");
    printf("            (every file at the smallest of 16, 20, 24, 32 bits that holds its samples exactly, probed on the GPU; no --dither)\n");
    printf("\n");
}

// the command line into `o`; false (after the usage text or the line that says why) where alacconvert exits with 1
inline bool parse_args(int argc, char **argv, Options &o)
{
    bool malformed = argc < 2;
    for (int i = 1; i < argc && !malformed; i++) {
        const std::string a = argv[i];
        const bool more = i + 1 < argc;  // an option that needs a value and is the last word is an unknown option
        if (a == "-h") {
            malformed = true;
        } else if (a == "--batch") {
            o.batch = true;
        } else if (a == "--lpc") {
            o.lpc = true;
        } else if (a == "--verify") {
            o.verify = true;
        } else if (a == "--verify-source") {
            o.verifySource = true;
        } else if (a == "--compare") {
            o.compare = true;
        } else if (a == "--crc") {
            o.crc = true;
        } else if (a == "--loudness") {
            o.loudness = true;
        } else if (a == "--true-peak") {
            o.truePeak = true;
        } else if (a == "--crc-check" && more) {
            o.crcList = argv[++i];
            malformed = o.crcList.empty();
        } else if (a == "--segment-packets" && more) {
            o.segmentPackets = (uint32_t)strtoul(argv[++i], nullptr, 10);
            malformed = o.segmentPackets == 0;
        } else if (a == "--float-bits" && more) {
            o.floatAuto = std::string(argv[++i]) == "auto";
            o.floatBits = o.floatAuto ? 0 : (uint32_t)strtoul(argv[i], nullptr, 10);
            malformed = !o.floatAuto && !pcm_depth_ok(o.floatBits);
        } else if (a == "--bits") {
            o.bitsNamed = true;
            if (!more) {
                malformed = true;
                continue;
            }
            o.intAuto = std::string(argv[++i]) == "auto";
            o.intBits = o.intAuto ? 0 : (uint32_t)strtoul(argv[i], nullptr, 10);
            if (!o.intAuto && !pcm_depth_ok(o.intBits)) {
                fprintf(stderr, " --bits takes 16, 20, 24, 32 or auto, not \"%s\"\n", argv[i]);
                return false;
            }
        } else if (a == "--dither") {
            o.dither.on = true;
        } else if (a == "--dither-seed" && more) {
            char *end = nullptr;
            o.dither.seed = strtoull(argv[++i], &end, 0);  // decimal or 0x-hex
            malformed = end == argv[i] || *end;
        } else if (a == "--rate" && more) {
            o.rate = (uint32_t)strtoul(argv[++i], nullptr, 10);
            malformed = o.rate == 0;
        } else if (a == "--devices" && more) {
            o.devices = (uint32_t)strtoul(argv[++i], nullptr, 10);
            malformed = o.devices == 0;
        } else if (!a.empty() && a[0] == '-') {
            printf("unknown option: %s\n", a.c_str());  // main.cu:92-96
            malformed = true;
        } else {
            o.files.push_back(a);
        }
    }
    const size_t n = o.files.size();
    const bool crcMode = o.crc || !o.crcList.empty();
    if (o.loudness) {
        // --loudness stands alone (but --devices N and --true-peak): any number of inputs, no output files
        if (malformed || n == 0 || crcMode || o.compare || o.dither.on || o.dither.seed || o.bitsNamed || o.batch || o.lpc ||
            o.verify || o.verifySource || o.segmentPackets || o.floatInput() || o.intConvert() || o.rate) {
            usage();
            return false;
        }
        return true;
    }
    if (o.truePeak) {  // --true-peak adds a column to the lines of --loudness: nothing without it
        usage();
        return false;
    }
    // --rate goes with an encode alone, at a depth the command line or the file fixes: not with --bits, --float-bits auto, a
    // verification (the PCM or floats to compare with are those of the other rate) or a mode that only prints
    if (o.rate && (o.bitsNamed || o.floatAuto || o.verify || o.verifySource || o.compare || crcMode)) malformed = true;
    if (!malformed && o.bitsNamed && (o.floatInput() || o.compare || crcMode)) {
        fprintf(stderr, " --bits converts integer PCM in front of an encode: not with %s\n",
                o.floatInput() ? "--float-bits" : o.compare ? "--compare" : o.crc ? "--crc" : "--crc-check");
        return false;
    }
    // neither --crc / --crc-check nor --compare goes with one of these
    const bool converting =
        o.batch || o.lpc || o.verify || o.verifySource || o.segmentPackets || o.floatInput() || o.intConvert() || o.rate;
    if (crcMode) {
        // --crc and --crc-check stand alone (but --devices N): any number of inputs resp. one list, no output files
        malformed = malformed || converting || o.compare || o.dither.on || (o.crc && !o.crcList.empty()) || (o.crc ? n == 0 : n != 0);
    } else {
        malformed = malformed || n < 2 || (n & 1) || (!o.batch && n != 2);
        malformed = malformed || (o.devices && !o.batch);  // one file is one serial chain: nothing to deal out
    }
    // --compare stands alone: two files, no other option
    // (but --dither [--dither-seed S], for a float reference of a file that was encoded with it)
    malformed = malformed || (o.compare && (converting || o.devices));
    if (malformed) {
        usage();
        if (o.bitsNamed) usage_bits();
        return false;
    }
    if (crcMode || o.compare) return true;
    if (o.dither.on && o.intConvert() && (o.intAuto || o.intBits == 32)) {  // auto promises lossless: no dither there
        fprintf(stderr, " --dither needs --bits 16, 20 or 24\n");
        usage();
        usage_bits();
        return false;
    }
    if (o.intConvert() && o.verifySource) {
        fprintf(stderr, " --verify-source needs float input (--float-bits N); with --bits, --verify checks against the converted PCM\n");
        return false;
    }
    if (o.dither.on && !o.intConvert() && (o.floatBits == 0 || o.floatBits == 32)) {  // auto promises lossless: no dither there
        fprintf(stderr, " --dither needs --float-bits 16, 20 or 24\n");
        usage();
        return false;
    }
    if (o.verifySource && !o.floatInput()) {
        fprintf(stderr, " --verify-source needs float input (--float-bits N); --verify checks an integer encode: \"%s\"\n", o.files[0].c_str());
        return false;
    }
    if (o.floatInput() && o.verify) {
        fprintf(stderr, " --verify does not take float input (--float-bits): \"%s\"\n", o.files[0].c_str());
        return false;
    }
    return true;
}

// ---- a group of files of one format as one run of packets ----
struct PacketCut {
    std::vector<uint32_t> numSamples;   // sample-frames of every packet
    std::vector<uint32_t> firstPacket;  // per file, and the packet count behind the last: file j is [firstPacket[j], firstPacket[j + 1])
    std::vector<uint32_t> segments;     // first packet of every segment, and the packet count behind the last
};

// The reference cuts a file's payload into full packets plus one partial one (main.cu:476-545) and drops a trailing
// fraction of a frame (ALACEncoder.cu:984).  Every file starts a segment (the predictor state is not carried from file to
// file); with segmentPackets != 0 so does every segmentPackets-th packet of a file.
inline PacketCut cut_packets(const std::vector<uint64_t> &dataBytes, uint32_t bytesPerFrame, uint32_t frame, uint32_t segmentPackets)
{
    const uint64_t packetBytes = (uint64_t)bytesPerFrame * frame;
    PacketCut cut;
    cut.segments.push_back(0);
    for (size_t j = 0; j < dataBytes.size(); j++) {
        const uint64_t full = dataBytes[j] / packetBytes, rest = dataBytes[j] - full * packetBytes;
        const uint32_t p0 = (uint32_t)cut.numSamples.size();
        cut.firstPacket.push_back(p0);
        cut.numSamples.insert(cut.numSamples.end(), (size_t)full, frame);
        if (rest) cut.numSamples.push_back((uint32_t)(rest / bytesPerFrame));
        const uint32_t p1 = (uint32_t)cut.numSamples.size();
        // a file without payload is an empty segment, which the segment table cannot hold
        for (uint32_t p = p0 + segmentPackets; segmentPackets && p < p1; p += segmentPackets) cut.segments.push_back(p);
        if (p1 != cut.segments.back()) cut.segments.push_back(p1);
    }
    cut.firstPacket.push_back((uint32_t)cut.numSamples.size());
    return cut;
}

// ---- files to workers ----
struct Part {
    size_t group;
    std::vector<size_t> members;  // indices into the group, ascending
};

// The members of every group dealt round-robin to the workers, the deal continuing where the last group stopped.  Per worker:
// the parts it takes, in group order.
inline std::vector<std::vector<Part> > deal(const std::vector<size_t> &groupSizes, uint32_t workers)
{
    std::vector<std::vector<Part> > perWorker(workers);
    size_t next = 0;
    for (size_t g = 0; g < groupSizes.size(); g++) {
        for (size_t m = 0; m < groupSizes[g]; m++, next++) {
            std::vector<Part> &mine = perWorker[next % workers];
            if (mine.empty() || mine.back().group != g) mine.push_back(Part{g, {}});
            mine.back().members.push_back(m);
        }
    }
    return perWorker;
}

// fn(k) for every worker k: a call where there is one, else one host thread each (nothing is shared between them)
template <class F>
void run_workers(uint32_t workers, F fn)
{
    if (workers == 1) {
        fn(0u);
        return;
    }
    std::vector<std::thread> threads;
    for (uint32_t k = 0; k < workers; k++) threads.emplace_back(fn, k);
    for (size_t k = 0; k < threads.size(); k++) threads[k].join();
}

// "%08x  <frames>  <path>", a line of --crc: the path is everything behind the second pair of blanks
inline bool parse_crc_line(const std::string &line, uint32_t &crc, uint64_t &frames, std::string &path)
{
    const size_t a = line.find("  "), b = a == std::string::npos ? a : line.find("  ", a + 2);
    if (a != 8 || b == std::string::npos || b + 2 >= line.size()) return false;
    char *endCrc = nullptr, *endFrames = nullptr;
    crc = (uint32_t)strtoul(line.c_str(), &endCrc, 16);
    frames = strtoull(line.c_str() + a + 2, &endFrames, 10);
    path = line.substr(b + 2);
    return endCrc == line.c_str() + a && endFrames == line.c_str() + b;
}

}  // namespace plan

#endif
