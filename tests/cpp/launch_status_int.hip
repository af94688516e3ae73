// launch_status_int.hip — launch_pcm_requantize (alac_amd/csrc/alac_pcm_in.hip, compiled into this program with the host
// side sanitized) hands back a status for everything it is asked.  What it refuses itself (a depth, a container or a source
// width it has no kernel for; dither where nothing is rounded) comes back as hipErrorInvalidValue with nothing enqueued,
// device or not.  Where there is NO GPU every path is then called once with null device pointers, which the launcher only
// passes on: the runtime fails cleanly, no kernel runs, and each call must hand that failure back.  With a device present
// that second part is left out, and the program never calls into the HIP runtime (tests/test_launch_status_int.py).
#include <cstdio>

#include <unistd.h>

#include "alac_kernels.hpp"

using namespace alacdev;

static int g_bad = 0;

static void expect(const char *what, hipError_t e, bool wantInvalid)
{
    const bool ok = wantInvalid ? e == hipErrorInvalidValue : e != hipSuccess;
    printf("%-58s hipError_t %d%s\n", what, (int)e, ok ? "" : "   <-- unexpected");
    if (!ok) g_bad++;
}

static PcmInArgs source(uint32_t cb, uint32_t bits, uint32_t channels, bool planar, uint32_t frame)
{
    PcmInArgs a{};
    a.channelStride = planar ? 64ull * frame : 1;
    a.frameStride = planar ? 1 : channels;
    a.numPackets = 64;
    a.frameSize = frame;
    a.channels = channels;
    a.containerBytes = cb;
    a.srcBits = bits;
    a.leftJustified = 1;
    return a;
}

int main()
{
    hipStream_t st = nullptr;
    const FloatDitherArgs dz{};
    expect("depth 18", launch_pcm_requantize(18, source(4, 24, 2, true, 4096), st), true);
    expect("container of 5 bytes", launch_pcm_requantize(16, source(5, 24, 2, true, 4096), st), true);
    expect("container of 1 byte", launch_pcm_requantize(16, source(1, 16, 2, true, 4096), st), true);
    expect("22 significant bits", launch_pcm_requantize(16, source(4, 22, 2, true, 4096), st), true);
    expect("24 bits in 2 bytes", launch_pcm_requantize(16, source(2, 24, 2, true, 4096), st), true);
    expect("dither, 16 -> 16", launch_pcm_requantize(16, source(2, 16, 2, true, 4096), st, &dz), true);
    expect("dither, 24 -> 24", launch_pcm_requantize(24, source(4, 24, 2, true, 4096), st, &dz), true);
    expect("dither, 16 -> 32", launch_pcm_requantize(32, source(4, 16, 2, true, 4096), st, &dz), true);
    PcmInArgs none = source(4, 24, 2, true, 4096);
    none.numPackets = 0;
    if (launch_pcm_requantize(16, none, st) != hipSuccess) {
        printf("no packets: not hipSuccess\n");
        g_bad++;
    }

    // (where the driver's device node exists the runtime is not even asked: nothing above has called into it, and a sanitized
    // host program has no business initialising a GPU)
    int devices = 0;
    if (access("/dev/kfd", F_OK) == 0 || (hipGetDeviceCount(&devices) == hipSuccess && devices > 0)) {
        printf("a device is present: the calls with null device pointers are left out\n");
    } else {
        uint32_t *clipped = (uint32_t *)(uintptr_t)4096;  // never touched: the memset in front of the launch fails first
        for (uint32_t depth : {16u, 20u, 24u, 32u})
            for (uint32_t cb : {2u, 3u, 4u})
                for (int path = 0; path < 4; path++) {  // mono, planar stereo, interleaved stereo, general (6 channels, frame 17)
                    if (cb == 3 && path == 1) continue;  // two rows of packed 3-byte containers take the general path
                    PcmInArgs a = path == 3 ? source(cb, 8 * cb == 32 ? 32 : 8 * cb, 6, true, 17)
                                            : source(cb, 8 * cb, path == 0 ? 1 : 2, path != 2, 4096);
                    char what[96];
                    snprintf(what, sizeof what, "%u bits from %u-byte containers, path %d", depth, cb, path);
                    expect(what, launch_pcm_requantize(depth, a, st), false);
                    a.clipped = clipped;
                    expect(what, launch_pcm_requantize(depth, a, st), false);
                    if (depth < 8 * cb) expect(what, launch_pcm_requantize(depth, a, st, &dz), false);
                }
    }
    if (g_bad)
        printf("%d calls did not answer as expected\n", g_bad);
    else
        printf("every call answered as expected\n");
    return g_bad ? 1 : 0;
}
