// alac_host.hpp — host-buffer staging shared by the C-ABI (alac_capi.hip), the classes (ALACEncoder.cpp, ALACDecoder.cpp)
// and the stage shims (alac_stage_compat.cpp, alac_matrix.hip).  Internal: not installed.  A staging step reports a failure
// through `fail(code, what, hipError)`, which returns the status the caller hands back (the C-ABI keeps the message too).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "alac_hip.h"

namespace alachost {

// one device allocation, freed with its owner (teardown: hipFree's status is not checked)
struct DevBuf {
    void *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(uint64_t n) { return hipMalloc(&p, n ? n : 4); }
};

// the packets back to back (+ 16 bytes of slack) and their offsets, the prefix sum of the sizes, staged on `st`
struct DevStream {
    DevBuf bytes, offs;
    uint64_t total = 0;  // stream bytes
};
template <class Fail>
int32_t upload_stream(const uint8_t *h_stream, const uint32_t *h_packet_bytes, uint32_t num_packets, hipStream_t st,
                      DevStream &d, Fail fail)
{
    std::vector<uint64_t> offs(num_packets + 1, 0);
    for (uint32_t i = 0; i < num_packets; i++) offs[i + 1] = offs[i] + h_packet_bytes[i];
    d.total = offs[num_packets];
    hipError_t e;
    if ((e = d.bytes.alloc(d.total + 16)) || (e = d.offs.alloc((num_packets + 1) * 8ull)))
        return fail(ALAC_HIP_MemFullError, "hipMalloc", e);
    if ((e = hipMemcpyAsync(d.bytes.p, h_stream, d.total, hipMemcpyHostToDevice, st)) ||
        (e = hipMemcpyAsync(d.offs.p, offs.data(), (num_packets + 1) * 8ull, hipMemcpyHostToDevice, st)))
        return fail(ALAC_HIP_ParamError, "H2D copy", e);
    return ALAC_HIP_noErr;
}

// The caller's side of a host encode call: what is staged in and where the results go.  What a call does not use stays null.
struct HostEncode {
    const uint32_t *numSamples;
    uint32_t numPackets;
    const uint32_t *segFirst;
    uint32_t numSegments;
    int16_t *state;  // nullable: gets the state back; read first where stateIn is set
    int32_t stateIn;
    uint8_t *out;
    uint64_t outCapacity;
    uint32_t *packetBytes;
    uint64_t *outTotalBytes = nullptr;  // nullable: the bytes of the stream, on success
    uint32_t *clipped = nullptr;  // these two of a float or integer source: staged by alac_capi.hip itself
    const uint64_t *packetOrigin = nullptr;
};

// the device side encode_host_common has staged for `launch`; maxSeg: the longest segment of the host table
struct StagedEncode {
    uint32_t maxSeg;
    const uint32_t *numSamples, *segFirst;
    int16_t *state;
    int32_t stateIn;
    void *ws;
    uint8_t *out;
    uint64_t outCapacity;
    uint32_t *packetBytes;
    uint64_t *offsets;
};

// The encode calls over host tables: the tables and the state staged to the device, `launch` (the device call on the staged
// buffers: const StagedEncode & -> status), the results copied back, then `wait` (the wait and the hand-off check of the
// context -> status).  wsBytes: the device call's workspace.
template <class Launch, class Fail, class Wait>
int32_t encode_host_common(hipStream_t st, const alac_hip_format *fmt, const HostEncode &h, uint64_t wsBytes, Launch launch,
                           Fail fail, Wait wait)
{
    const uint32_t np = h.numPackets, nseg = h.numSegments;
    const uint64_t stateBytes = (uint64_t)nseg * alac_hip_state_int16(fmt) * 2;
    const uint64_t outMax = alac_hip_encode_max_output_bytes(fmt, np);
    const bool stIn = h.state && h.stateIn;

    DevBuf dNs, dSeg, dState, dWs, dOut, dSizes, dOffs;
    hipError_t e;
    if ((e = dNs.alloc(np * 4ull)) || (e = dSeg.alloc((nseg + 1) * 4ull)) || (e = dState.alloc(stateBytes)) ||
        (e = dWs.alloc(wsBytes)) || (e = dOut.alloc(outMax)) || (e = dSizes.alloc(np * 4ull)) ||
        (e = dOffs.alloc((np + 1) * 8ull)))
        return fail(ALAC_HIP_MemFullError, "hipMalloc", e);
    if ((e = hipMemcpyAsync(dNs.p, h.numSamples, np * 4ull, hipMemcpyHostToDevice, st)) ||
        (e = hipMemcpyAsync(dSeg.p, h.segFirst, (nseg + 1) * 4ull, hipMemcpyHostToDevice, st)))
        return fail(ALAC_HIP_ParamError, "H2D copy", e);
    if (stIn && (e = hipMemcpyAsync(dState.p, h.state, stateBytes, hipMemcpyHostToDevice, st)))
        return fail(ALAC_HIP_ParamError, "H2D state", e);
    uint32_t maxSeg = 1;
    for (uint32_t s = 0; s < nseg; s++)
        maxSeg = h.segFirst[s + 1] - h.segFirst[s] > maxSeg ? h.segFirst[s + 1] - h.segFirst[s] : maxSeg;
    if (int32_t rc = launch(StagedEncode{maxSeg, (const uint32_t *)dNs.p, (const uint32_t *)dSeg.p, (int16_t *)dState.p,
                                         stIn ? 1 : 0, dWs.p, (uint8_t *)dOut.p, outMax, (uint32_t *)dSizes.p, (uint64_t *)dOffs.p}))
        return rc;
    uint64_t total = 0;
    if ((e = hipMemcpyAsync(&total, (uint64_t *)dOffs.p + np, 8, hipMemcpyDeviceToHost, st)) || (e = hipStreamSynchronize(st)))
        return fail(ALAC_HIP_ParamError, "encode execution", e);
    if (total > h.outCapacity) return fail(ALAC_HIP_MemFullError, "host output buffer too small", hipSuccess);
    if ((e = hipMemcpyAsync(h.out, dOut.p, total, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h.packetBytes, dSizes.p, np * 4ull, hipMemcpyDeviceToHost, st)))
        return fail(ALAC_HIP_ParamError, "D2H copy", e);
    if (h.state && (e = hipMemcpyAsync(h.state, dState.p, stateBytes, hipMemcpyDeviceToHost, st)))
        return fail(ALAC_HIP_ParamError, "D2H state", e);
    if (int32_t rc = wait()) return rc;
    if (h.outTotalBytes) *h.outTotalBytes = total;
    return ALAC_HIP_noErr;
}

}  // namespace alachost
