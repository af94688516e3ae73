// alac_verify.hip — the two small kernels around a verify pass (alac_hip_verify).  The comparison itself happens at the
// decoders' PCM store sites (alac_verify.hpp); these set the per-packet minima up and turn them into the answer.
#include "alac_kernels.hpp"

namespace alacdev {

__global__ __launch_bounds__(256) void k_verify_init(uint32_t *firstMismatch, uint32_t n, uint32_t *bad)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) firstMismatch[i] = 0xffffffffu;
    if (i == 0) *bad = 0;
}

// per packet: a status other than 0 -> 0 (nothing of it decoded); a decoded frame count other than the expected one ->
// min(decoded, expected) unless an earlier frame differs (frames behind the shorter count were never compared: the store
// sites compare only what the decoder produced, and a frame at or behind min(decoded, expected) cannot lower the minimum
// below it); then one ballot and one atomic per wave for the count of failed packets
__global__ __launch_bounds__(256) void k_verify_finish(const int32_t *status, const uint32_t *nsDec, const uint32_t *nsExp,
                                                       uint32_t frameSize, uint32_t n, uint32_t *firstMismatch, uint32_t *bad)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool failed = false;
    if (i < n) {
        uint32_t fm = firstMismatch[i];
        const uint32_t d = nsDec[i], e = nsExp ? nsExp[i] : frameSize;
        if (status[i] != 0) fm = 0;
        else if (d != e) fm = min(fm, min(d, e));
        firstMismatch[i] = fm;
        failed = fm != 0xffffffffu;
    }
    const uint64_t m = __ballot(failed);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(bad, (uint32_t)__popcll(m));
}

hipError_t launch_verify_init(uint32_t *firstMismatch, uint32_t numPackets, uint32_t *bad, hipStream_t st)
{
    const uint32_t blocks = numPackets ? (numPackets + 255) / 256 : 1;
    return launch_kernel(k_verify_init, dim3(blocks), dim3(256), st, firstMismatch, numPackets, bad);
}

hipError_t launch_verify_finish(const int32_t *status, const uint32_t *numSamplesDecoded, const uint32_t *numSamplesExpected,
                                uint32_t frameSize, uint32_t numPackets, uint32_t *firstMismatch, uint32_t *bad, hipStream_t st)
{
    if (numPackets == 0) return hipSuccess;
    return launch_kernel(k_verify_finish, dim3((numPackets + 255) / 256), dim3(256), st, status, numSamplesDecoded, numSamplesExpected,
                         frameSize, numPackets, firstMismatch, bad);
}

}  // namespace alacdev
