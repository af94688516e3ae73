// alac_pcm_crc.hip — alac_hip_pcm_crc32: one streaming pass over a byte buffer that gives the CRC-32 (zlib's: polynomial
// 0xEDB88320 reflected, initial value and final XOR 0xFFFFFFFF) of every range of a table.  Reads the plane alac_hip_decode
// writes and writes only the digests.
//
// The arithmetic is GF(2)[x] / P on reflected words: bit 31 is x^0, x^8 is 0x00800000, crc_mul multiplies.  pure(A) is the
// register after A with initial value 0 and no final XOR; it is linear in A, and (include/alac_hip.h)
//     pure(A || B) = pure(A) * x^(8|B|) ^ pure(B)          crc32(A) = pure(A) ^ 0xFFFFFFFF * x^(8|A|) ^ 0xFFFFFFFF
// so the bytes of a range may be hashed in any pieces: a piece whose last byte lies d bytes in front of the range's end adds
// pure(piece) * x^(8d) to the range's word, and XOR does not care in which order the pieces arrive.
#include "alac_dev.hpp"
#include "alac_kernels.hpp"

#include <cstring>

namespace alacdev {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;  // x^0

// a * b mod P: 32 shift-and-xor steps (gfx950 has no carry-less multiply).  Not on the per-16-byte path.
__host__ __device__ inline uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll 4
    for (int i = 31; i >= 0; i--) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return p;
}

// x^(8 * 2^k), k < 64: computed on the host once
static const uint32_t *crc_pow8_table()
{
    static uint32_t table[64];
    static const bool ready = [] {
        uint32_t v = 0x00800000u;  // x^8
        for (int k = 0; k < 64; k++) {
            table[k] = v;
            v = crc_mul(v, v);
        }
        return true;
    }();
    (void)ready;
    return table;
}

uint32_t crc_mul_host(uint32_t a, uint32_t b) { return crc_mul(a, b); }

uint32_t crc_x8_pow(uint64_t bytes)
{
    const uint32_t *t = crc_pow8_table();
    uint32_t v = kCrcOne;
    for (int k = 0; bytes; k++, bytes >>= 1)
        if (bytes & 1) v = crc_mul(v, t[k]);
    return v;
}

struct PcmCrcKernelArgs {
    const uint8_t *base;     // the buffer's start rounded down to 16 bytes: positions below count from here
    uint64_t shift;          // what that rounding added to every offset of the caller
    uint64_t lo, hi;         // first byte of the first range, end of the last one (positions)
    const uint64_t *ranges;  // device table of {offset, length} in the CALLER's offsets; null: the one range [lo, hi)
    uint32_t numRanges;
    uint32_t xPass;          // x^(8 * bytes between two iterations of a block's grid-stride loop)
    uint32_t *digests;       // 4 words per range (alac_hip_pcm_digest); word 2 collects the pure register
    uint32_t pow8[64];
};

// LDS of a block: the slicing tables sl[j][b] = b * x^(8(j + 1)) (byte b of a 16-byte group that j more bytes follow), the
// tables adv[j][b] = (b << 8j) * xPass that move a register over one iteration's stride, and x^(8 * 2^k)
struct CrcLds {
    uint32_t sl[16][256];
    uint32_t adv[4][256];
    uint32_t pow8[64];
};

__device__ __forceinline__ void crc_build_tables(CrcLds &L, const PcmCrcKernelArgs &a)
{
    const uint32_t b = threadIdx.x;  // 256 threads: one entry of every table each
    uint32_t c = b;
#pragma unroll
    for (int i = 0; i < 8; i++) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
    L.sl[0][b] = c;
#pragma unroll
    for (int j = 0; j < 4; j++) L.adv[j][b] = crc_mul(b << (8 * j), a.xPass);
    if (b < 64) L.pow8[b] = a.pow8[b];
    __syncthreads();
    for (int j = 1; j < 16; j++) {
        c = L.sl[0][c & 0xff] ^ (c >> 8);  // one more zero byte behind it
        L.sl[j][b] = c;
    }
    __syncthreads();
}

// the register r run over the 16 bytes of v: the 16 lookups are independent, only the XOR into r is serial
__device__ __forceinline__ uint32_t crc_group16(const CrcLds &L, uint32_t r, const uint4 v)
{
    const uint32_t w0 = v.x ^ r;
    return L.sl[15][w0 & 0xff] ^ L.sl[14][(w0 >> 8) & 0xff] ^ L.sl[13][(w0 >> 16) & 0xff] ^ L.sl[12][w0 >> 24] ^
           L.sl[11][v.y & 0xff] ^ L.sl[10][(v.y >> 8) & 0xff] ^ L.sl[9][(v.y >> 16) & 0xff] ^ L.sl[8][v.y >> 24] ^
           L.sl[7][v.z & 0xff] ^ L.sl[6][(v.z >> 8) & 0xff] ^ L.sl[5][(v.z >> 16) & 0xff] ^ L.sl[4][v.z >> 24] ^
           L.sl[3][v.w & 0xff] ^ L.sl[2][(v.w >> 8) & 0xff] ^ L.sl[1][(v.w >> 16) & 0xff] ^ L.sl[0][v.w >> 24];
}

// v * x^(8 * bytes): square-and-multiply over the table
__device__ __forceinline__ uint32_t crc_shift(const CrcLds &L, uint32_t v, uint64_t bytes)
{
    for (uint32_t k = 0; bytes; k++, bytes >>= 1)
        if (bytes & 1) v = crc_mul(v, L.pow8[k]);
    return v;
}

// range s as positions [rs, re)
__device__ __forceinline__ void crc_range(const PcmCrcKernelArgs &a, uint32_t s, uint64_t &rs, uint64_t &re)
{
    if (a.ranges) {
        rs = a.ranges[2 * s] + a.shift;
        re = rs + a.ranges[2 * s + 1];
    } else {
        rs = a.lo, re = a.hi;
    }
}

// the largest s whose range starts at or in front of position p (p >= lo; the offsets ascend, so empty ranges that start
// where a later one does are passed over)
__device__ __forceinline__ uint32_t crc_range_of(const PcmCrcKernelArgs &a, uint64_t p)
{
    uint32_t lo = 0, hi = a.numRanges;
    if (!a.ranges) return 0;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.ranges[2 * mid] + a.shift <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

// a piece of range s whose last byte lies `behind` bytes in front of the range's end
__device__ __forceinline__ void crc_emit(const CrcLds &L, const PcmCrcKernelArgs &a, uint32_t s, uint32_t r, uint64_t behind)
{
    if (r) atomicXor(a.digests + 4ull * s + 2, crc_shift(L, r, behind));
}

// the accumulators of a wave, lane l's counted to the end of its own chunk, as one value counted to the end of lane 63's:
// step k multiplies the lower partner by x^(8 * kCrcLaneBytes * 2^k) (lane 63 gets the result)
__device__ __forceinline__ uint32_t crc_wave_reduce(const CrcLds &L, uint32_t v, uint32_t lane)
{
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const uint32_t lower = __shfl_xor(v, 1 << k);
        const uint32_t moved = crc_mul(lower, L.pow8[kPcmCrcLaneShift + k]);
        v = (lane >> k) & 1 ? v ^ moved : v;
    }
    return v;
}

constexpr uint64_t kCrcNoPos = ~0ull;

// One lane: the kPcmCrcLaneBytes (64) consecutive bytes at a multiple of 64 from a.base, four 16-byte loads; a wave: 4 096
// bytes; a block: 16 384; a grid-stride loop over the blocks that cover [lo, hi).
// A wave whose 4 096 bytes all lie in one range (uniform: the range is found by a binary search on wave-uniform values) hashes
// its chunks with the slicing tables into per-lane accumulators that live across the loop: the next iteration of the block
// lies a.xPass further, the accumulator is moved there with four lookups and the new chunk's register is XORed in.  They go
// out — one wave reduction, one move to the range's end, one atomicXor — when the wave leaves the range or skips an
// iteration, and at the end of the kernel.  Any other wave (a range boundary, the call's first and last bytes, a gap) takes
// the per-lane path: every lane walks the bytes of its chunk that lie in ranges one by one, and sends one atomicXor per
// piece.  Bytes outside every range form no address.
__global__ __launch_bounds__(256) void k_pcm_crc(PcmCrcKernelArgs a)
{
    __shared__ CrcLds L;
    crc_build_tables(L, a);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t firstBlock = a.lo / kPcmCrcBlockBytes;
    const uint64_t totalBlocks = (a.hi + kPcmCrcBlockBytes - 1) / kPcmCrcBlockBytes - firstBlock;
    uint32_t acc = 0, accRange = 0;
    uint64_t accPos = kCrcNoPos, accEnd = 0;  // the wave's first byte in the last iteration it accumulated; its range's end
    for (uint64_t vb = blockIdx.x; vb < totalBlocks; vb += gridDim.x) {
        const uint64_t fw = (firstBlock + vb) * kPcmCrcBlockBytes + wave * kPcmCrcWaveBytes;  // the wave's first byte
        if (fw >= a.hi || fw + kPcmCrcWaveBytes <= a.lo) continue;                              // (wave-uniform)
        uint32_t s = 0;
        uint64_t rs = a.lo, re = a.hi;
        bool uniform = fw >= a.lo;
        if (uniform) {
            s = crc_range_of(a, fw);
            crc_range(a, s, rs, re);
            uniform = fw + kPcmCrcWaveBytes <= re;
        }
        const uint64_t c0 = fw + lane * kPcmCrcLaneBytes;
        if (uniform) {
            const uint4 *g = (const uint4 *)(a.base + c0);
            const uint4 v0 = g[0], v1 = g[1], v2 = g[2], v3 = g[3];
            const bool follows = accPos != kCrcNoPos && s == accRange &&
                                 fw == accPos + (uint64_t)gridDim.x * kPcmCrcBlockBytes;
            if (!follows) {
                if (accPos != kCrcNoPos) {
                    const uint32_t w = crc_wave_reduce(L, acc, lane);
                    if (lane == 63) crc_emit(L, a, accRange, w, accEnd - (accPos + kPcmCrcWaveBytes));
                }
                acc = 0;
                accRange = s, accEnd = re;
            }
            accPos = fw;
            uint32_t r = crc_group16(L, 0, v0);
            r = crc_group16(L, r, v1);
            r = crc_group16(L, r, v2);
            r = crc_group16(L, r, v3);
            acc = L.adv[0][acc & 0xff] ^ L.adv[1][(acc >> 8) & 0xff] ^ L.adv[2][(acc >> 16) & 0xff] ^ L.adv[3][acc >> 24] ^ r;
        } else {
            uint64_t p = c0 > a.lo ? c0 : a.lo;
            const uint64_t stop = c0 + kPcmCrcLaneBytes < a.hi ? c0 + kPcmCrcLaneBytes : a.hi;
            if (p >= stop) continue;
            uint32_t ls = crc_range_of(a, p);
            for (;;) {
                uint64_t ps, pe;
                crc_range(a, ls, ps, pe);
                if (p >= pe) {  // behind this range (or it is empty): the next one
                    if (++ls >= a.numRanges) break;
                    continue;
                }
                p = p < ps ? ps : p;  // a gap
                if (p >= stop) break;
                const uint64_t e = pe < stop ? pe : stop;
                uint32_t r = 0;
                for (; p < e; p++) r = L.sl[0][(r ^ a.base[p]) & 0xff] ^ (r >> 8);
                crc_emit(L, a, ls, r, pe - e);
            }
        }
    }
    if (accPos != kCrcNoPos) {
        const uint32_t w = crc_wave_reduce(L, acc, lane);
        if (lane == 63) crc_emit(L, a, accRange, w, accEnd - (accPos + kPcmCrcWaveBytes));
    }
}

// per range: the length term and the final XOR onto the collected register, and the other fields of the record
__global__ __launch_bounds__(256) void k_pcm_crc_finish(PcmCrcKernelArgs a)
{
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.numRanges) return;
    const uint64_t len = a.ranges ? a.ranges[2 * s + 1] : a.hi - a.lo;
    uint32_t v = 0xFFFFFFFFu;
    uint64_t n = len;
    for (uint32_t k = 0; n; k++, n >>= 1)
        if (n & 1) v = crc_mul(v, a.pow8[k]);
    uint32_t *d = a.digests + 4ull * s;
    const uint32_t pure = d[2];
    d[0] = (uint32_t)len, d[1] = (uint32_t)(len >> 32);
    d[2] = pure ^ v ^ 0xFFFFFFFFu;
    d[3] = 0;
}

// blocks of a launch (the tests' PASS is kPcmCrcBlockBytes times this).  Not tuned: 1 024 blocks of 20.5 KB LDS are 4 waves
// per SIMD, as k_float_probe runs.
constexpr uint32_t kPcmCrcMaxBlocks = 1024;

hipError_t launch_pcm_crc(const PcmCrcArgs &c, hipStream_t st)
{
    if (c.numRanges == 0) return hipErrorInvalidValue;
    ALAC_TRY(hipMemsetAsync(c.digests, 0, (uint64_t)c.numRanges * 16, st));
    PcmCrcKernelArgs a;
    a.shift = (uintptr_t)c.pcm & 15;
    a.base = c.pcm - a.shift;
    a.lo = c.lo + a.shift, a.hi = c.hi + a.shift;
    a.ranges = c.ranges;
    a.numRanges = c.numRanges;
    a.digests = c.digests;
    memcpy(a.pow8, crc_pow8_table(), sizeof(a.pow8));
    uint32_t grid = 1;
    if (a.hi > a.lo) {
        const uint64_t blocks = (a.hi + kPcmCrcBlockBytes - 1) / kPcmCrcBlockBytes - a.lo / kPcmCrcBlockBytes;
        grid = (uint32_t)(blocks < kPcmCrcMaxBlocks ? blocks : kPcmCrcMaxBlocks);
    }
    a.xPass = crc_x8_pow((uint64_t)grid * kPcmCrcBlockBytes);
    if (a.hi > a.lo) ALAC_TRY(launch_kernel(k_pcm_crc, dim3(grid), dim3(256), st, a));
    return launch_kernel(k_pcm_crc_finish, dim3((c.numRanges + 255) / 256), dim3(256), st, a);
}

}  // namespace alacdev
