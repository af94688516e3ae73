// The pure pieces of alacconvert (convert-utility/plan.h) against literal expectations worked out by hand from the tool's
// rules: the packet cut, the deal of files to workers, a line of a --crc list, the command line.  Host only; built with
// the address and undefined-behaviour sanitizers (tests/cpp/Makefile) and run by tests/test_convert_plan.py.
#include <cstdio>
#include <cstdlib>

#include "plan.h"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            exit(1);                                                  \
        }                                                             \
    } while (0)

typedef std::vector<uint32_t> U32;
typedef std::vector<size_t> Idx;

static bool parse(std::vector<const char *> words, plan::Options &o)
{
    words.insert(words.begin(), "alacconvert");
    return plan::parse_args((int)words.size(), const_cast<char **>(words.data()), o);
}

static void test_cut_packets()
{
    // no payload; two full packets, 77 frames and three stray bytes (the dropped fraction of a frame); one full packet
    const std::vector<uint64_t> files = {0, 2 * 4096 * 4 + 77 * 4 + 3, 4096 * 4};
    const U32 segments[3] = {{0, 3, 4}, {0, 1, 2, 3, 4}, {0, 2, 3, 4}};  // segmentPackets 0, 1, 2
    for (uint32_t k = 0; k < 3; k++) {
        const plan::PacketCut cut = plan::cut_packets(files, 4, 4096, k);
        CHECK(cut.numSamples == (U32{4096, 4096, 77, 4096}));
        CHECK(cut.firstPacket == (U32{0, 0, 3, 4}));
        CHECK(cut.segments == segments[k]);
    }
    const plan::PacketCut none = plan::cut_packets({0}, 4, 4096, 0);
    CHECK(none.numSamples.empty() && none.firstPacket == (U32{0, 0}) && none.segments == (U32{0}));
}

static void test_deal()
{
    const std::vector<std::vector<plan::Part> > w = plan::deal({3, 2, 2}, 3);
    CHECK(w.size() == 3);
    // worker 0: group 0 member 0, group 1 member 0, group 2 member 1
    CHECK(w[0].size() == 3 && w[0][0].group == 0 && w[0][0].members == (Idx{0}) && w[0][1].group == 1 &&
          w[0][1].members == (Idx{0}) && w[0][2].group == 2 && w[0][2].members == (Idx{1}));
    // worker 1: group 0 member 1, group 1 member 1
    CHECK(w[1].size() == 2 && w[1][0].group == 0 && w[1][0].members == (Idx{1}) && w[1][1].group == 1 &&
          w[1][1].members == (Idx{1}));
    // worker 2: group 0 member 2, group 2 member 0
    CHECK(w[2].size() == 2 && w[2][0].group == 0 && w[2][0].members == (Idx{2}) && w[2][1].group == 2 &&
          w[2][1].members == (Idx{0}));
    const std::vector<std::vector<plan::Part> > one = plan::deal({3, 2, 2}, 1);
    CHECK(one.size() == 1 && one[0].size() == 3);
    CHECK(one[0][0].group == 0 && one[0][0].members == (Idx{0, 1, 2}));
    CHECK(one[0][1].group == 1 && one[0][1].members == (Idx{0, 1}));
    CHECK(one[0][2].group == 2 && one[0][2].members == (Idx{0, 1}));
    const std::vector<std::vector<plan::Part> > few = plan::deal({1, 1}, 4);  // workers that get nothing
    CHECK(few.size() == 4 && few[0].size() == 1 && few[1].size() == 1 && few[1][0].group == 1 && few[2].empty() && few[3].empty());
    const std::vector<std::vector<plan::Part> > none = plan::deal({}, 2);
    CHECK(none.size() == 2 && none[0].empty() && none[1].empty());

    // run_workers: every worker once, with its own index
    for (uint32_t workers : {1u, 3u}) {
        std::vector<int> calls(workers, 0);
        plan::run_workers(workers, [&](uint32_t k) { calls[k]++; });
        CHECK(calls == std::vector<int>(workers, 1));
    }
}

static void test_parse_crc_line()
{
    uint32_t crc = 0;
    uint64_t frames = 0;
    std::string path;
    CHECK(plan::parse_crc_line("0123abcd  77  a  b.wav", crc, frames, path));
    CHECK(crc == 0x0123abcdu && frames == 77 && path == "a  b.wav");
    for (const char *bad : {"123abcd  77  p", "0123abcd 77 p", "0123abcd  77  ", "0123abcd  77", "0123abcd  7x  p", "0123abcg  77  p", ""})
        CHECK(!plan::parse_crc_line(bad, crc, frames, path));
}

static void test_parse_args()
{
    plan::Options pair;
    CHECK(parse({"in.wav", "out.caf"}, pair));
    CHECK(pair.files == (std::vector<std::string>{"in.wav", "out.caf"}));
    CHECK(!pair.batch && !pair.lpc && !pair.verify && !pair.verifySource && !pair.compare && !pair.crc && pair.crcList.empty());
    CHECK(!pair.segmentPackets && !pair.devices && !pair.floatBits && !pair.floatAuto && !pair.floatInput() && !pair.dither.on);

    plan::Options batch;
    CHECK(parse({"--batch", "--devices", "2", "a", "b", "c", "d"}, batch));
    CHECK(batch.batch && batch.devices == 2 && batch.files == (std::vector<std::string>{"a", "b", "c", "d"}));
    CHECK(!batch.lpc && !batch.verify && !batch.floatInput() && !batch.crc);

    plan::Options source;
    CHECK(parse({"--float-bits", "auto", "--verify-source", "a", "b"}, source));
    CHECK(source.floatAuto && source.floatBits == 0 && source.floatInput() && source.verifySource && !source.verify);

    plan::Options seed;
    CHECK(parse({"--float-bits", "16", "--dither", "--dither-seed", "0x10", "a", "b"}, seed));
    CHECK(seed.dither.on && seed.dither.seed == 16 && seed.floatBits == 16 && !seed.floatAuto);
}

static void test_small_spellings()
{
    for (uint32_t bits = 0; bits <= 40; bits++) CHECK(plan::pcm_depth_ok(bits) == (bits == 16 || bits == 20 || bits == 24 || bits == 32));
    CHECK(plan::bytes_per_sample(16) == 2 && plan::bytes_per_sample(20) == 3 && plan::bytes_per_sample(24) == 3 &&
          plan::bytes_per_sample(32) == 4);
}

int main()
{
    test_cut_packets();
    test_deal();
    test_parse_crc_line();
    test_parse_args();
    test_small_spellings();
    printf("ok\n");
    return 0;
}
