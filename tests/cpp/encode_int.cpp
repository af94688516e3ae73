// ALACEncoder::EncodeSegmentsInt and the host forms of the integer C-ABI driven from a test (tests/test_gpu_encode_int.py)
//   encode_int <dir> <frame size> <depth> <channels> <container bytes> <bits> <left justified> <channel stride>
//              <frame stride> <dither mode> <seed>
// reads <dir>/in (the containers), <dir>/counts (uint32 per packet), <dir>/segs (uint32 segment table) and, where it exists,
// <dir>/origin (uint64 per packet); writes <dir>/stream, <dir>/sizes, <dir>/clipped (the class), <dir>/pcm and
// <dir>/pcm_clipped (alac_hip_pcm_requantize_host on a context of its own).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "ALACEncoder.h"
#include "alac_hip.h"

static std::vector<uint8_t> slurp(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void dump(const std::string &path, const void *p, size_t n)
{
    std::ofstream(path, std::ios::binary).write((const char *)p, (std::streamsize)n);
}

int main(int argc, char **argv)
{
    if (argc != 12) return 2;
    const std::string dir = argv[1];
    const uint32_t frame = (uint32_t)atoi(argv[2]), depth = (uint32_t)atoi(argv[3]), channels = (uint32_t)atoi(argv[4]);
    const alac_hip_int_source src = {(uint32_t)atoi(argv[5]),  (uint32_t)atoi(argv[6]),  (uint32_t)atoi(argv[7]), 0,
                                     strtoull(argv[8], nullptr, 10), strtoull(argv[9], nullptr, 10)};
    const alac_hip_dither dither = {(uint32_t)atoi(argv[10]), 0, strtoull(argv[11], nullptr, 10)};
    const std::vector<uint8_t> in = slurp(dir + "/in"), countBytes = slurp(dir + "/counts"), segBytes = slurp(dir + "/segs"),
                               originBytes = slurp(dir + "/origin");
    const uint32_t np = (uint32_t)(countBytes.size() / 4), nseg = (uint32_t)(segBytes.size() / 4) - 1;
    const uint32_t *counts = (const uint32_t *)countBytes.data(), *segs = (const uint32_t *)segBytes.data();
    const uint64_t *origin = originBytes.empty() ? nullptr : (const uint64_t *)originBytes.data();

    ALACEncoder enc;
    enc.SetFrameSize(frame);
    enc.SetDither(dither.mode, dither.seed);
    AudioFormatDescription f;
    memset(&f, 0, sizeof(f));
    f.mFormatID = kALACFormatAppleLossless;
    f.mSampleRate = 44100;
    f.mFormatFlags = depth == 16 ? 1 : depth == 20 ? 2 : depth == 24 ? 3 : 4;
    f.mFramesPerPacket = frame;
    f.mChannelsPerFrame = channels;
    if (enc.InitializeEncoder(f, 0) != ALAC_noErr) return 3;
    const alac_hip_format fmt = {frame, depth, channels, 44100};
    std::vector<uint8_t> out(alac_hip_encode_max_output_bytes(&fmt, np));
    std::vector<uint32_t> sizes(np), clipped(np);
    uint64_t total = 0;
    int32_t rc = enc.EncodeSegmentsInt(in.data(), src, counts, np, segs, nseg, out.data(), out.size(), sizes.data(), &total,
                                       clipped.data(), origin);
    if (rc != 0) {
        fprintf(stderr, "EncodeSegmentsInt: status %d\n", rc);
        return 4;
    }
    dump(dir + "/stream", out.data(), total);
    dump(dir + "/sizes", sizes.data(), np * 4ull);
    dump(dir + "/clipped", clipped.data(), np * 4ull);

    alac_hip_ctx *ctx = nullptr;
    if (alac_hip_create(&ctx, 0, nullptr) != ALAC_HIP_noErr) return 5;
    const uint32_t bps = depth == 16 ? 2 : depth == 32 ? 4 : 3;
    std::vector<uint8_t> pcm((uint64_t)np * frame * channels * bps);
    rc = alac_hip_pcm_requantize_host(ctx, &fmt, in.data(), &src, counts, np, pcm.data(), pcm.size(), clipped.data(), &dither,
                                      origin);
    if (rc != 0) {
        fprintf(stderr, "alac_hip_pcm_requantize_host: status %d (%s)\n", rc, alac_hip_last_error(ctx));
        return 6;
    }
    dump(dir + "/pcm", pcm.data(), pcm.size());
    dump(dir + "/pcm_clipped", clipped.data(), np * 4ull);
    alac_hip_destroy(ctx);
    return 0;
}
