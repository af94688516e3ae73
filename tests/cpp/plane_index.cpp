// The index rule of the encoder's residual planes (alac_amd/csrc/alac_plane_index.hpp, host build) enumerated: for every
// stride the map (sample, stream) -> int32 index is a bijection onto the whole cells of the plane, a chain's four samples
// of a group are contiguous and 16-byte aligned, and consecutive streams are 16 bytes apart (tests/test_plane_index.py).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "alac_plane_index.hpp"

using namespace alacdev;

static int failures = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (failures++ < 20) {               \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);        \
                std::printf("\n");               \
            }                                    \
        }                                        \
    } while (0)

int main()
{
    const uint64_t rows = 70;
    const uint64_t strides[] = {64, 320, 5 * 64};
    for (uint64_t stride : strides) {
        CHECK(plane_rows(rows) == 72, "plane_rows(70) = %llu", (unsigned long long)plane_rows(rows));
        const uint64_t size = kPlaneGroup * stride * (plane_rows(rows) / kPlaneGroup);
        std::vector<uint8_t> hit(size, 0);
        for (uint64_t j = 0; j < plane_rows(rows); j++)
            for (uint64_t s = 0; s < stride; s++) {
                const uint64_t i = plane_index(j, stride, s);
                CHECK(i < size, "index %llu of (%llu, %llu) outside the plane", (unsigned long long)i, (unsigned long long)j,
                      (unsigned long long)s);
                if (i >= size) continue;
                CHECK(!hit[i], "index %llu hit twice", (unsigned long long)i);
                hit[i] = 1;
                if ((j & 3) == 0) {
                    CHECK((i * 4) % 16 == 0, "group of (%llu, %llu) not 16-byte aligned", (unsigned long long)j, (unsigned long long)s);
                    for (uint64_t k = 1; k < 4; k++)
                        CHECK(plane_index(j + k, stride, s) == i + k, "group of (%llu, %llu) not contiguous", (unsigned long long)j,
                              (unsigned long long)s);
                }
                if (s + 1 < stride)
                    CHECK((plane_index(j, stride, s + 1) - i) * 4 == 16, "streams %llu, %llu + 1 not 16 bytes apart",
                          (unsigned long long)s, (unsigned long long)s);
                // a sub-plane that starts at stream `first` indexes the same cell
                const uint64_t first = s / 2;
                int32_t *const base = nullptr;
                CHECK(plane_from_stream(base, first) + plane_index(j, stride, s - first) == base + i, "plane_from_stream(%llu)",
                      (unsigned long long)first);
            }
        for (uint64_t i = 0; i < size; i++) CHECK(hit[i], "index %llu never hit (stride %llu)", (unsigned long long)i, (unsigned long long)stride);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
