// alac_lpc.hip — the opt-in LPC encode mode (option "lpc"): every packet is independent, and each channel of a packet may
// carry predictor coefficients computed from the packet's own PCM instead of Apple's init_coefs.
//
// Runs after the regular pipeline has encoded every packet as its own segment (Apple's independent packet: mix decision,
// numU / numV, bit strings, escape decision in the PacketRec).  One workgroup per packet, three waves per channel:
//   1. the channel's plane (mixed with the packet's mixRes, low bytes shifted off) into LDS
//   2. autocorrelation, lags 0..30, in double: thread t of the channel sums the samples j = t (mod 192), then a fixed
//      butterfly per wave and the three waves in order — the reduction order depends on the packet alone
//   3. Levinson-Durbin (one lane, double) -> candidate orders 4, 8, 12, 16, 24, 30; coefficient k-1 = round(a_k 2^den),
//      den the largest <= 15 for which every coefficient fits int16.  Dropped: r[0] == 0, an unstable recursion
//      (|k_m| >= 1 or a non-positive error), den < 5 (outside the exact range of the tap-parallel predictor), and
//      orders with 2 * order >= numSamples
//   4. exact trial count: each half-wave runs one candidate through the adaptive predictor (alac_taps.hpp, pc_block's
//      general loop) and the Golomb coder (alac_golomb.hpp) in counting mode
//   5. per channel the cheapest of {Apple's channel, the candidates} (header 16 * num + bits); where a candidate wins,
//      its half-wave runs again and writes the channel's bit string over Apple's, and the packet record and size are
//      updated.  Escaped packets stay escaped; a packet can only get smaller than Apple's independent packet.
// The packer (alac_encode.hip k_pack) takes the header of an LPC channel from LpcChan.
#include "alac_dev.hpp"
#include "alac_golomb.hpp"
#include "alac_kernels.hpp"
#include "alac_taps.hpp"

namespace alacdev {

using namespace taps;

namespace {

constexpr int kLags = kLpcMaxOrder + 1;
constexpr int kCands = 6;
constexpr int kWavesPerChan = 3;  // six half-waves: one per candidate
constexpr int kChanThreads = 64 * kWavesPerChan;
__constant__ int kOrders[kCands] = {4, 8, 12, 16, 24, 30};

struct Cand {
    int32_t den;  // 0: dropped
    int16_t coefs[32];
};

// One pass of a candidate over the plane X (N samples, LDS) by a whole half-wave; every lane ends with the same count.
// WRITE: the bit string goes to `slot` (all lanes of the half store the same words).
template <bool WRITE>
__device__ uint32_t lpc_pass(const int32_t *X, uint32_t N, const Cand &cd, int na, int k, uint32_t chanBits,
                             const uint32_t *recip, uint32_t *slot, uint32_t wcap)
{
    const uint32_t chanshift = 32 - chanBits;
    int32_t a = k < na ? (int32_t)cd.coefs[k] : 0;
    int32_t x = 0;
    GolF g;
    golf_reset(g);
    if constexpr (WRITE) golf_open(g, slot, wcap);
    for (uint32_t j = 0; j < N; j++) {
        const int32_t cur = X[j];
        int32_t del;
        if (j > (uint32_t)na) {
            del = taps_step(cur, x, a, na, k, chanshift, (uint32_t)cd.den);
        } else {
            // warm-up positions (dp_enc.c:90, :108-112): the first sample, then first differences
            const int32_t prev = __shfl(x, 0, 32);
            del = j == 0 ? cur : sext(cur - prev, chanshift);
        }
        x = taps_slide(x, cur, k);
        if constexpr (WRITE)
            if ((j & 15) == 0) g.wp = g.wp < g.wlim ? g.wp : g.wlim;  // capacity guard (golf_stream's, per 16 symbols)
        golf_sym<WRITE, false>(g, del, true, chanBits, recip);
    }
    golf_finish<WRITE>(g, N > 0, recip);
    if constexpr (WRITE) {
        golf_flush<WRITE>(g);
        return golf_written_bits(g, slot);
    }
    return g.bits;
}

// Levinson-Durbin over r[0..30] into the candidate table (one lane).  The arithmetic is pinned for the host reference
// (oracle/lpc_ref.py): the three fused steps are explicit fma() calls, and nothing else may be contracted.
__device__ void lpc_levinson(const double *r, uint32_t N, Cand *cand)
{
#pragma clang fp contract(off)
    for (int c = 0; c < kCands; c++) cand[c].den = 0;
    if (!(r[0] > 0.0)) return;
    double a[kLags] = {0}, t[kLags];
    double err = r[0];
    int next = 0;
    for (int m = 1; m <= kLpcMaxOrder && next < kCands; m++) {
        double acc = r[m];
        for (int i = 1; i < m; i++) acc = fma(-a[i], r[m - i], acc);
        const double km = acc / err;
        if (!(fabs(km) < 1.0)) return;
        for (int i = 1; i < m; i++) t[i] = fma(-km, a[m - i], a[i]);
        for (int i = 1; i < m; i++) a[i] = t[i];
        a[m] = km;
        err *= fma(-km, km, 1.0);
        if (!(err > 0.0)) return;
        if (m != kOrders[next]) continue;
        Cand &cd = cand[next++];
        if (2u * (uint32_t)m >= N) return;
        double amax = 0;
        for (int i = 1; i <= m; i++) amax = fmax(amax, fabs(a[i]));
        int den = 15;
        while (den >= 5 && rint(amax * (double)(1 << den)) > 32767.0) den--;
        if (den < 5) continue;
        for (int i = 1; i <= m; i++) cd.coefs[i - 1] = (int16_t)rint(a[i] * (double)(1 << den));
        cd.den = den;
    }
}

}  // namespace

template <int DEPTH, int CH>
__global__ __launch_bounds__(kChanThreads * CH) void k_lpc(LpcArgs A)
{
    extern __shared__ int32_t planes[];  // [CH][frameSize]
    __shared__ uint32_t recip[17];
    __shared__ double part[CH][kWavesPerChan][kLags];
    __shared__ Cand cand[CH][kCands];
    __shared__ uint32_t bits[CH][kCands];
    __shared__ int32_t win[CH];
    constexpr uint32_t SHB = bytes_shifted(DEPTH);
    constexpr uint32_t chanBits = DEPTH - 8 * SHB + (CH == 2 ? 1 : 0);
    const uint32_t p = blockIdx.x, tid = threadIdx.x;
    const uint32_t c = tid / kChanThreads, tc = tid - c * kChanThreads, wave = tc >> 6, lane = tc & 63;
    const int k = (int)(lane & 31), h = (int)(wave * 2 + (lane >> 5));  // candidate of this half-wave
    PacketRec *rec = A.recs + p;
    if (tid < CH) A.lpc[(uint64_t)p * 2 + tid].num = 0;  // 0: the packer writes Apple's header for the channel
    const uint32_t N = rec->numSamples, mixRes = rec->mixRes;
    if (rec->escape || N == 0 || N > A.frameSize) return;
    gol_table_init(recip, (int)tid);
    int32_t *X = planes + c * A.frameSize;
    const uint8_t *pk = A.pcm + (uint64_t)p * A.frameSize * CH * bytes_per_sample(DEPTH);
    for (uint32_t j = tc; j < N; j += kChanThreads) {
        if constexpr (CH == 2) {
            int32_t l, r;
            load_lr<DEPTH>(pk, j, l, r);
            X[j] = mix_sample((int32_t)mixRes, (int)c, l, r);
        } else {
            X[j] = load_sample<DEPTH>(pk, j) >> (8 * (int)SHB);
        }
    }
    __syncthreads();

    // autocorrelation
    double acc[kLags];
#pragma unroll
    for (int L = 0; L < kLags; L++) acc[L] = 0.0;
    for (uint32_t j = tc; j < N; j += kChanThreads) {
        const double xj = (double)X[j];
#pragma unroll
        for (int L = 0; L < kLags; L++)
            if (j >= (uint32_t)L) acc[L] = fma(xj, (double)X[j - L], acc[L]);
    }
#pragma unroll
    for (int L = 0; L < kLags; L++) {
        double v = acc[L];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if (lane == 0) part[c][wave][L] = v;
    }
    __syncthreads();
    if (tc == 0) {
        double r[kLags];
        for (int L = 0; L < kLags; L++) r[L] = (part[c][0][L] + part[c][1][L]) + part[c][2][L];
        lpc_levinson(r, N, cand[c]);
    }
    __syncthreads();

    // exact trial counts, one candidate per half-wave
    const Cand &cd = cand[c][h];
    const int na = kOrders[h];
    const bool live = cd.den != 0;
    if (live) {
        const uint32_t b = lpc_pass<false>(X, N, cd, na, k, chanBits, recip, nullptr, 0);
        if (k == 0) bits[c][h] = b;
    }
    __syncthreads();
    if (tc == 0) {
        uint32_t best = 16u * rec->c[c].num + rec->c[c].bits;  // Apple's channel
        int w = -1;
        for (int q = 0; q < kCands; q++) {
            if (!cand[c][q].den) continue;
            const uint32_t cost = 16u * (uint32_t)kOrders[q] + bits[c][q];
            if (cost < best) best = cost, w = q;
        }
        win[c] = w;
    }
    __syncthreads();
    if (win[c] == h) {
        uint32_t *slot = A.bitWords + ((uint64_t)p * 2 + c) * A.wcap;
        const uint32_t b = lpc_pass<true>(X, N, cd, na, k, chanBits, recip, slot, A.wcap);
        if (k == 0) {
            rec->c[c].bits = b;
            rec->c[c].num = (uint16_t)na;
            LpcChan &o = A.lpc[(uint64_t)p * 2 + c];
            o.den = (uint16_t)cd.den;
            for (int i = 0; i < na; i++) o.coefs[i] = cd.coefs[i];
            o.num = (uint16_t)na;
        }
    }
    __syncthreads();
    if (tid == 0 && (win[0] >= 0 || win[CH - 1] >= 0)) {
        // k_finalize's size for a compressed packet (the packet was compressed and only got smaller)
        const uint32_t partial = (N != A.frameSize);
        uint32_t body = 12 + 4 + (partial ? 32 : 0) + 16 + N * (SHB * 8) * CH;
        for (uint32_t q = 0; q < (uint32_t)CH; q++) body += 16 + 16 * rec->c[q].num + rec->c[q].bits;
        rec->totalBits = 7 + body + 3;
        A.packetBytes[p] = (7 + body + 3 + 7) / 8;
    }
}

template <int DEPTH>
static hipError_t launch_lpc_depth(uint32_t channels, const LpcArgs &a, uint32_t numPackets, hipStream_t st)
{
    const size_t lds = (size_t)channels * a.frameSize * 4;
    if (channels == 2) return launch_kernel_lds(k_lpc<DEPTH, 2>, dim3(numPackets), dim3(2 * kChanThreads), lds, st, a);
    return launch_kernel_lds(k_lpc<DEPTH, 1>, dim3(numPackets), dim3(kChanThreads), lds, st, a);
}

hipError_t launch_lpc(uint32_t depth, uint32_t channels, const LpcArgs &a, uint32_t numPackets, hipStream_t st)
{
    if (numPackets == 0) return hipSuccess;
    switch (depth) {
    case 16: return launch_lpc_depth<16>(channels, a, numPackets, st);
    case 20: return launch_lpc_depth<20>(channels, a, numPackets, st);
    case 24: return launch_lpc_depth<24>(channels, a, numPackets, st);
    case 32: return launch_lpc_depth<32>(channels, a, numPackets, st);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace alacdev
