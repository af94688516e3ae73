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

// The encode calls over host tables: the tables and the state staged to the device, `launch` (the device call on the staged
// buffers: (maxSeg, num samples, segment table, state, state_in, workspace, out, out capacity, sizes, offsets) -> status),
// the results copied back, then `wait` (the wait and the hand-off check of the context -> status).  wsBytes: the device
// call's workspace; h_state (nullable) gets the state back; *out_total_bytes (nullable): the bytes of the stream, on success.
template <class Launch, class Fail, class Wait>
int32_t encode_host_common(hipStream_t st, const alac_hip_format *fmt, const uint32_t *h_num_samples, uint32_t num_packets,
                           const uint32_t *h_seg_first, uint32_t num_segments, int16_t *h_state, int32_t state_in,
                           uint8_t *h_out, uint64_t out_capacity, uint32_t *h_packet_bytes, uint64_t *out_total_bytes,
                           uint64_t wsBytes, Launch launch, Fail fail, Wait wait)
{
    const uint32_t np = num_packets, nseg = num_segments;
    const uint64_t stateBytes = (uint64_t)nseg * alac_hip_state_int16(fmt) * 2;
    const uint64_t outMax = alac_hip_encode_max_output_bytes(fmt, np);
    const bool stIn = h_state && state_in;

    DevBuf dNs, dSeg, dState, dWs, dOut, dSizes, dOffs;
    hipError_t e;
    if ((e = dNs.alloc(np * 4ull)) || (e = dSeg.alloc((nseg + 1) * 4ull)) || (e = dState.alloc(stateBytes)) ||
        (e = dWs.alloc(wsBytes)) || (e = dOut.alloc(outMax)) || (e = dSizes.alloc(np * 4ull)) ||
        (e = dOffs.alloc((np + 1) * 8ull)))
        return fail(ALAC_HIP_MemFullError, "hipMalloc", e);
    if ((e = hipMemcpyAsync(dNs.p, h_num_samples, np * 4ull, hipMemcpyHostToDevice, st)) ||
        (e = hipMemcpyAsync(dSeg.p, h_seg_first, (nseg + 1) * 4ull, hipMemcpyHostToDevice, st)))
        return fail(ALAC_HIP_ParamError, "H2D copy", e);
    if (stIn && (e = hipMemcpyAsync(dState.p, h_state, stateBytes, hipMemcpyHostToDevice, st)))
        return fail(ALAC_HIP_ParamError, "H2D state", e);
    uint32_t maxSeg = 1;
    for (uint32_t s = 0; s < nseg; s++)
        maxSeg = h_seg_first[s + 1] - h_seg_first[s] > maxSeg ? h_seg_first[s + 1] - h_seg_first[s] : maxSeg;
    if (int32_t rc = launch(maxSeg, (const uint32_t *)dNs.p, (const uint32_t *)dSeg.p, (int16_t *)dState.p, stIn ? 1 : 0,
                            dWs.p, (uint8_t *)dOut.p, outMax, (uint32_t *)dSizes.p, (uint64_t *)dOffs.p))
        return rc;
    uint64_t total = 0;
    if ((e = hipMemcpyAsync(&total, (uint64_t *)dOffs.p + np, 8, hipMemcpyDeviceToHost, st)) || (e = hipStreamSynchronize(st)))
        return fail(ALAC_HIP_ParamError, "encode execution", e);
    if (total > out_capacity) return fail(ALAC_HIP_MemFullError, "host output buffer too small", hipSuccess);
    if ((e = hipMemcpyAsync(h_out, dOut.p, total, hipMemcpyDeviceToHost, st)) ||
        (e = hipMemcpyAsync(h_packet_bytes, dSizes.p, np * 4ull, hipMemcpyDeviceToHost, st)))
        return fail(ALAC_HIP_ParamError, "D2H copy", e);
    if (h_state && (e = hipMemcpyAsync(h_state, dState.p, stateBytes, hipMemcpyDeviceToHost, st)))
        return fail(ALAC_HIP_ParamError, "D2H state", e);
    if (int32_t rc = wait()) return rc;
    if (out_total_bytes) *out_total_bytes = total;
    return ALAC_HIP_noErr;
}

}  // namespace alachost
