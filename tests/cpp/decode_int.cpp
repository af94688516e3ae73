// ALACDecoder::DecodeBatchInt driven from a test (tests/test_gpu_decode_int_class.py): the packets of a 24-bit stream in
//   decode_int <cookie file> <stream file> <packet sizes file (uint32)>
// DecodeBatch gives the packed bytes; DecodeBatchInt must give, in three layouts, what the host unpacks from them: planar int32
// left-justified with a gap behind each row, interleaved int32 right-justified (the containers of a 24-in-32 file), and
// interleaved packed 3-byte containers (the bytes themselves).  Prints "ok <frames> <containers compared>", or the first
// difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static int32_t sample24(const uint8_t *p)
{
    const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    return (int32_t)(v << 8) >> 8;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    std::vector<uint8_t> cookie = slurp(argv[1]), stream = slurp(argv[2]), sizeBytes = slurp(argv[3]);
    const uint32_t np = (uint32_t)(sizeBytes.size() / 4);
    const uint32_t *sizes = (const uint32_t *)sizeBytes.data();
    ALACDecoder dec;
    if (dec.Init(cookie.data(), (uint32_t)cookie.size(), 0) != 0) return 3;
    const uint32_t ch = dec.mConfig.numChannels, frame = dec.mConfig.frameLength;
    if (dec.mConfig.bitDepth != 24) return 3;
    const uint64_t T = (uint64_t)np * frame;

    std::vector<uint8_t> bytes(T * ch * 3, 0);
    std::vector<uint32_t> frames(np, 0), framesInt(np, 0);
    std::vector<int32_t> status(np, 7), statusInt(np, 7);
    int32_t rc = dec.DecodeBatch(stream.data(), sizes, np, bytes.data(), frames.data(), status.data());
    if (rc != 0) {
        fprintf(stderr, "DecodeBatch: status %d\n", rc);
        return 4;
    }
    uint64_t total = 0, compared = 0;
    for (uint32_t p = 0; p < np; p++) total += frames[p];

    auto counts_ok = [&](const char *what) {
        for (uint32_t p = 0; p < np; p++)
            if (framesInt[p] != frames[p] || statusInt[p] != status[p]) {
                printf("%s: packet %u: %u frames, status %d; DecodeBatch %u, %d\n", what, p, framesInt[p], statusInt[p], frames[p],
                       status[p]);
                return false;
            }
        return true;
    };

    // planar int32, left-justified, 5 containers of gap behind each row
    {
        const uint64_t stride = T + 5;
        const int32_t kGap = 0x5A5A5A5A;
        std::vector<int32_t> out(ch * stride, kGap);
        const alac_hip_int_dest dst = {4, 32, 1, 0, stride, 1};
        rc = dec.DecodeBatchInt(stream.data(), sizes, np, out.data(), &dst, framesInt.data(), statusInt.data());
        if (rc != 0 || !counts_ok("planar")) {
            fprintf(stderr, "DecodeBatchInt (planar): status %d\n", rc);
            return 4;
        }
        for (uint32_t c = 0; c < ch; c++) {
            for (uint64_t t = 0; t < T; t++, compared++) {
                const int32_t want = (int32_t)((uint32_t)sample24(&bytes[(t * ch + c) * 3]) << 8);
                if (out[c * stride + t] != want) {
                    printf("planar: channel %u frame %llu: %d, expected %d\n", c, (unsigned long long)t, out[c * stride + t], want);
                    return 1;
                }
            }
            for (uint64_t t = T; t < stride; t++)
                if (out[c * stride + t] != kGap) {
                    printf("planar: the gap behind row %u was written\n", c);
                    return 1;
                }
        }
    }
    // interleaved int32, right-justified at 24 bits
    {
        std::vector<int32_t> out(T * ch, -1);
        const alac_hip_int_dest dst = {4, 24, 0, 0, 1, ch};
        rc = dec.DecodeBatchInt(stream.data(), sizes, np, out.data(), &dst, framesInt.data(), statusInt.data());
        if (rc != 0 || !counts_ok("interleaved")) {
            fprintf(stderr, "DecodeBatchInt (interleaved): status %d\n", rc);
            return 4;
        }
        for (uint64_t i = 0; i < T * ch; i++, compared++)
            if (out[i] != sample24(&bytes[i * 3])) {
                printf("interleaved: container %llu: %d, expected %d\n", (unsigned long long)i, out[i], sample24(&bytes[i * 3]));
                return 1;
            }
    }
    // interleaved packed 3-byte containers: the identity descriptor
    {
        std::vector<uint8_t> out(T * ch * 3 + 3, 0xC3);
        const alac_hip_int_dest dst = {3, 24, 1, 0, 1, ch};
        rc = dec.DecodeBatchInt(stream.data(), sizes, np, out.data(), &dst, framesInt.data(), statusInt.data());
        if (rc != 0 || !counts_ok("packed")) {
            fprintf(stderr, "DecodeBatchInt (packed): status %d\n", rc);
            return 4;
        }
        if (memcmp(out.data(), bytes.data(), bytes.size()) != 0 || out[bytes.size()] != 0xC3 || out[bytes.size() + 2] != 0xC3) {
            printf("packed: the bytes differ from DecodeBatch's\n");
            return 1;
        }
        compared += T * ch;
    }
    // a reduction is refused
    {
        std::vector<int16_t> out(T * ch, 0x1111);
        const alac_hip_int_dest dst = {2, 16, 1, 0, T, 1};
        rc = dec.DecodeBatchInt(stream.data(), sizes, np, out.data(), &dst, framesInt.data(), statusInt.data());
        if (rc != kALAC_ParamError || out[0] != 0x1111 || out[T * ch - 1] != 0x1111) {
            printf("16-bit containers for a 24-bit stream: status %d, expected %d with nothing written\n", rc, kALAC_ParamError);
            return 1;
        }
    }
    printf("ok %llu %llu\n", (unsigned long long)total, (unsigned long long)compared);
    return 0;
}
