// launch_status.hip — every launcher of libalac_hip.so hands back the status of the runtime call that failed.
//
// Runs ONLY where there is no GPU: every launch and runtime call then fails cleanly (hipErrorNoDevice), no kernel ever runs,
// and the null device pointers below are never touched (the launchers only pass them on).  With a device present the program
// says so, does nothing else and exits 77 (tests/test_launch_status.py skips).  Argument blocks are zero-initialised, sizes
// are those of a small real batch: 64 packets of 16-bit stereo, frame 4096, one packet per segment.
#include <cstdio>
#include <cstring>

#include "alac_encode_v1_types.hpp"
#include "alac_hip.h"

using namespace alacdev;

static int g_bad = 0;

static void expect_failure(const char *what, hipError_t e)
{
    printf("%-44s %s\n", what, hipGetErrorName(e));
    if (e == hipSuccess) g_bad++;
}

int main()
{
    int devices = 0;
    if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) {
        printf("a device is present: this program only runs without one\n");
        return 77;
    }
    constexpr uint32_t N = 64, FRAME = 4096, DEPTH = 16, CH = 2;
    hipStream_t st = nullptr;

    expect_failure("launch_check_segments", launch_check_segments(nullptr, N, N, 1, nullptr, nullptr, st));

    EncodeArgs ea;
    memset(&ea, 0, sizeof(ea));
    ea.numSegments = ea.numPackets = N;
    ea.frameSize = FRAME;
    PackArgs pa{};
    pa.frameSize = FRAME;
    expect_failure("launch_encode", launch_encode(DEPTH, CH, ea, pa, N, st, nullptr));

    struct {
        const char *name;
        V1Shape shape;
        int32_t thru, narrow, fused, fold;
    } const plans[] = {
        {"launch_encode_v1 tiny", V1Shape::Tiny, -1, -1, 1, 1},
        {"launch_encode_v1 latency", V1Shape::Latency, -1, 0, 1, 1},
        {"launch_encode_v1 latency unfolded", V1Shape::LatencyUnfolded, -1, 0, 1, 0},
        {"launch_encode_v1 stagewise", V1Shape::Stagewise, -1, -1, 0, 1},
        {"launch_encode_v1 throughput", V1Shape::Throughput, 1, -1, 1, 1},
    };
    V1Args A;
    memset(&A, 0, sizeof(A));
    A.S.numSegments = A.S.segEnd = A.S.numPackets = N;
    A.S.frameSize = FRAME;
    A.chainsPad = N * CH;
    const V1Streams vs{};
    for (const auto &p : plans) {
        AlacOptions opt;
        opt.thru = p.thru;
        opt.narrow = p.narrow;
        opt.fused = p.fused;
        opt.fold = p.fold;
        const V1Plan P = v1_plan(CH, N, 1, FRAME, opt);
        if (P.shape != p.shape) {
            printf("%s: v1_plan chose %s\n", p.name, v1_regime_name(P.shape));
            g_bad++;
        }
        for (int initState = 0; initState < 2; initState++)
            expect_failure(p.name, launch_encode_v1(DEPTH, CH, A, P, initState != 0, pa, vs, N, 1, st, nullptr));
    }

    expect_failure("launch_scan_pack", launch_scan_pack(DEPTH, CH, nullptr, pa, N, st, nullptr));
    expect_failure("launch_scan_sizes", launch_scan_sizes(nullptr, nullptr, N, st));

    LpcArgs la{};
    la.frameSize = FRAME;
    expect_failure("launch_lpc", launch_lpc(DEPTH, CH, la, N, st));

    expect_failure("launch_mc_gather", launch_mc_gather(nullptr, nullptr, nullptr, N, FRAME, 6, 0, 2, 2, st));
    // (tables that are never read on the host: without one the launcher has nothing to do)
    const uint32_t *table = (const uint32_t *)(uintptr_t)4096;
    expect_failure("launch_mc_tables", launch_mc_tables(table, N, table, N, 2, nullptr, nullptr, st));
    McSpliceArgs sa{};
    sa.numElements = 4;
    sa.numPackets = N;
    expect_failure("launch_mc_splice", launch_mc_splice(sa, st));

    DecodeArgs da{};
    da.numPackets = N;
    da.frameSize = FRAME;
    da.bitDepth = DEPTH;
    da.numChannels = CH;
    da.maxElems = CH;
    const PcmModeArgs pm{};  // store mode has no words of its own
    expect_failure("launch_decode", launch_decode(da, pm, st));
    for (int32_t fused : {-1, 0}) {
        da.optFused = fused;
        expect_failure(fused ? "launch_decode_v1 dec_fused -1" : "launch_decode_v1 dec_fused 0",
                       launch_decode_v1(da, pm, nullptr, 0, nullptr, nullptr, st, nullptr));
    }
    da.optFused = -1;
    DecodeArgs d6 = da;
    d6.numChannels = d6.maxElems = 6;
    McElement el[kMaxChannels];
    const uint32_t nel = channel_elements(6, el);
    expect_failure("launch_decode_v1_elements",
                   launch_decode_v1_elements(d6, pm, el, nel, nullptr, 0, nullptr, nullptr, nullptr, nullptr, st));

    expect_failure("launch_verify_init", launch_verify_init(nullptr, N, nullptr, st));
    expect_failure("launch_verify_finish", launch_verify_finish(nullptr, nullptr, nullptr, FRAME, N, nullptr, nullptr, st));

    FloatInArgs fa{};
    fa.channelStride = (uint64_t)N * FRAME;
    fa.frameStride = 1;
    fa.numPackets = N;
    fa.frameSize = FRAME;
    fa.channels = CH;
    expect_failure("launch_float_to_pcm", launch_float_to_pcm(DEPTH, fa, st));
    FloatProbeArgs fp{};
    fp.channelStride = (uint64_t)N * FRAME;
    fp.frameStride = 1;
    fp.hi = (uint64_t)N * FRAME;
    fp.numSegments = 1;
    fp.channels = CH;
    expect_failure("launch_float_probe", launch_float_probe(fp, st));

    // 4 taps: one lane per row; 8 taps: the tap-parallel kernel
    expect_failure("launch_pc_block 4 taps", launch_pc_block(nullptr, nullptr, N, FRAME + 8, FRAME, nullptr, 4, 16, 9, false, st));
    expect_failure("launch_pc_block 8 taps", launch_pc_block(nullptr, nullptr, N, FRAME + 8, FRAME, nullptr, 8, 16, 9, false, st));
    if (!pc_block_taps_ok(FRAME, 8, 16, 9)) {
        printf("8 taps did not take the tap-parallel kernel\n");
        g_bad++;
    }
    expect_failure("launch_dyn_comp", launch_dyn_comp(10, 40, 14, nullptr, N, FRAME, FRAME, 16, nullptr, 0, nullptr, st));
    expect_failure("launch_dyn_decomp",
                   launch_dyn_decomp(10, 40, 14, nullptr, FRAME * 4, N, nullptr, FRAME, FRAME, 16, nullptr, nullptr, st));

    // the synth launcher needs a context, and there is none without a device: only its refusal can be seen from here
    alac_hip_ctx *ctx = nullptr;
    alac_hip_format fmt{};
    fmt.frame_size = FRAME;
    fmt.bit_depth = DEPTH;
    fmt.num_channels = CH;
    fmt.sample_rate = 44100;
    if (alac_hip_create(&ctx, 0, nullptr) == ALAC_HIP_noErr || alac_hip_synth_pcm(ctx, 0, N, &fmt, (uint8_t *)table) == ALAC_HIP_noErr) {
        printf("alac_hip_create / alac_hip_synth_pcm succeeded without a device\n");
        g_bad++;
    }

    if (g_bad)
        printf("%d calls did not report a failure\n", g_bad);
    else
        printf("every call reported a failure\n");
    return g_bad ? 1 : 0;
}
