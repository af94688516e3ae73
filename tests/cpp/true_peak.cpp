// ALACDecoder::LoudnessTruePeakBatch driven from a test (tests/test_gpu_alacconvert_true_peak.py), next to LoudnessBatch on the
// same packets: the packets of some files in, one line per file out
//   true_peak <cookie file> <stream file> <packet sizes file (uint32)> <first packet of every file, and the packet count (uint32)>
// prints "<lufs %.17g> <peak %.17g> <true peak %.17g> <lufs of LoudnessBatch %.17g> <peak of LoudnessBatch %.17g>" per file, then
// "frames <sum of the decoded frames>" and "bad <packets of non-zero status>"
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "ALACDecoder.h"
#include "alac_hip.h"

static std::vector<uint8_t> slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    std::vector<uint8_t> cookie = slurp(argv[1]), stream = slurp(argv[2]), sizeBytes = slurp(argv[3]), firstBytes = slurp(argv[4]);
    const uint32_t np = (uint32_t)(sizeBytes.size() / 4), numFiles = (uint32_t)(firstBytes.size() / 4) - 1;
    const uint32_t *sizes = (const uint32_t *)sizeBytes.data(), *first = (const uint32_t *)firstBytes.data();
    ALACDecoder dec;
    if (dec.Init(cookie.data(), (uint32_t)cookie.size(), 0) != 0) return 3;
    std::vector<double> lufs(numFiles), peak(numFiles), truePeak(numFiles, -1.0), lufs2(numFiles), peak2(numFiles);
    std::vector<uint32_t> frames(np, 0), frames2(np, 0);
    std::vector<int32_t> status(np, 0), status2(np, 0);
    int32_t rc = dec.LoudnessTruePeakBatch(stream.data(), sizes, np, first, numFiles, lufs.data(), peak.data(), truePeak.data(),
                                           frames.data(), status.data());
    if (rc != 0) {
        fprintf(stderr, "LoudnessTruePeakBatch: status %d\n", rc);
        return 4;
    }
    rc = dec.LoudnessBatch(stream.data(), sizes, np, first, numFiles, lufs2.data(), peak2.data(), frames2.data(), status2.data());
    if (rc != 0 || frames != frames2 || status != status2) {
        fprintf(stderr, "LoudnessBatch: status %d, or other frames or packet statuses\n", rc);
        return 5;
    }
    if (dec.LoudnessTruePeakBatch(stream.data(), sizes, np, first, numFiles, lufs.data(), peak.data(), nullptr, frames.data(),
                                  status.data()) != kALAC_ParamError)
        return 6;
    uint64_t total = 0, bad = 0;
    for (uint32_t p = 0; p < np; p++) total += frames[p], bad += status[p] != 0;
    for (uint32_t j = 0; j < numFiles; j++) printf("%.17g %.17g %.17g %.17g %.17g\n", lufs[j], peak[j], truePeak[j], lufs2[j], peak2[j]);
    printf("frames %llu\nbad %llu\n", (unsigned long long)total, (unsigned long long)bad);
    return 0;
}
