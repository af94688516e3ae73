// alac_hip_resample_int_host / alac_hip_resample_float_host driven from C++ (tests/test_gpu_resample_host.py): one stereo plane
// in, cut into two segments at frame <cut>, the float32 rows out
//   resample int|float <in rate> <out rate> <frames> <cut> <input file> <output file>
// int: 16-bit interleaved stereo; float: float32 planar, two rows of <frames>.  Writes the two output rows back to back and
// prints "<out_first> <out_frames> <peak %.17g> <nonfinite>" per segment, then "total <output frames of a row>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "alac_hip.h"

static std::vector<uint8_t> slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv)
{
    if (argc != 8) return 2;
    const bool isFloat = !strcmp(argv[1], "float");
    const uint32_t inRate = (uint32_t)atoi(argv[2]), outRate = (uint32_t)atoi(argv[3]);
    const uint64_t frames = strtoull(argv[4], nullptr, 10), cut = strtoull(argv[5], nullptr, 10);
    const std::vector<uint8_t> in = slurp(argv[6]);
    if (in.size() != frames * 2 * (isFloat ? 4 : 2)) return 3;
    const uint64_t table[3] = {0, cut, frames};
    uint64_t outFirst[3] = {0, 0, 0};
    const uint64_t total = alac_hip_resample_frames(inRate, outRate, frames, table, 2, outFirst);
    uint32_t L = 0, M = 0, K = 0;
    if (alac_hip_resample_filter(inRate, outRate, &L, &M, &K, nullptr) != 0) return 4;
    if (total != (cut * L + M - 1) / M + ((frames - cut) * L + M - 1) / M || outFirst[2] != total) return 5;
    alac_hip_ctx *ctx = nullptr;
    if (alac_hip_create(&ctx, 0, nullptr) != 0) return 6;
    std::vector<float> out(2 * total + 1, -7.25f);
    alac_hip_resample_report reports[2];
    int32_t rc;
    if (isFloat) {
        rc = alac_hip_resample_float_host(ctx, (const float *)in.data(), 2, frames, 1, inRate, outRate, frames, table, 2, out.data(),
                                          total, total, reports);
    } else {
        const alac_hip_int_source src = {2, 16, 1, 0, 1, 2};
        rc = alac_hip_resample_int_host(ctx, in.data(), &src, 2, inRate, outRate, frames, table, 2, out.data(), total, total,
                                        reports);
    }
    if (rc != 0) {
        fprintf(stderr, "resample host form: status %d: %s\n", rc, alac_hip_last_error(ctx));
        return 7;
    }
    // a row that is too short is refused and nothing is written
    std::vector<float> small(2 * total, 3.5f);
    alac_hip_resample_report untouched[2];
    memset(untouched, 0x5a, sizeof untouched);
    const alac_hip_int_source src16 = {2, 16, 1, 0, 1, 2};
    rc = isFloat ? alac_hip_resample_float_host(ctx, (const float *)in.data(), 2, frames, 1, inRate, outRate, frames, table, 2,
                                                small.data(), total, total - 1, untouched)
                 : alac_hip_resample_int_host(ctx, in.data(), &src16, 2, inRate, outRate, frames, table, 2, small.data(), total,
                                              total - 1, untouched);
    if (rc != ALAC_HIP_ParamError || small[0] != 3.5f || ((const uint8_t *)untouched)[0] != 0x5a) return 8;
    alac_hip_destroy(ctx);
    if (out[2 * total] != -7.25f) return 9;
    std::ofstream f(argv[7], std::ios::binary);
    f.write((const char *)out.data(), (std::streamsize)(2 * total * sizeof(float)));
    for (int s = 0; s < 2; s++)
        printf("%llu %llu %.17g %llu\n", (unsigned long long)reports[s].out_first, (unsigned long long)reports[s].out_frames,
               reports[s].peak, (unsigned long long)reports[s].nonfinite);
    printf("total %llu\n", (unsigned long long)total);
    return 0;
}
