/*
 * alac_hip.h — C-ABI of the MI355X-native ALAC hot path (libalac_hip.so).
 *
 * Plain pointers and sizes only.  Every entry point names the reference interface it replaces
 * (paths relative to the reference tree dark-Stallion/alac).  All `d_` pointers are device
 * (HBM) pointers on the context's device; `h_` pointers are host pointers.  Calls are enqueued on
 * the context's HIP stream and are asynchronous unless stated otherwise.  Return value is the
 * reference's int32 status convention: 0 = ALAC_noErr (codec/ALACBitUtilities.h:51-54),
 * -50 = kALAC_ParamError, -108 = kALAC_MemFullError, -4 = kALAC_UnimplementedError
 * (codec/ALACAudioTypes.h:54-60).  HIP runtime failures map to -108 (allocation) or -50.
 */
#ifndef ALAC_HIP_H
#define ALAC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    ALAC_HIP_noErr = 0,
    ALAC_HIP_UnimplementedError = -4,
    ALAC_HIP_ParamError = -50,
    ALAC_HIP_MemFullError = -108
};

/* Number of int16 values of persistent encoder state per segment and element: the predictor rows the
 * search touches, [U row 3][U row 7][V row 3][V row 7] x 16 coefficients — the live subset of
 * ALACEncoder::mCoefsU/V (codec/ALACEncoder.h:89-90, rows numUV-1 of codec/ALACEncoder.cu:361,429).
 * Mono and stereo streams have one element; a stream of 3..8 channels has one block per element of its
 * packets (mCoefsU/V[channelIndex] of the element's first channel), laid out [element][segment][64]:
 * alac_hip_state_int16(fmt) = 64 x elements is the per-segment total. */
#define ALAC_HIP_STATE_INT16 64

typedef struct alac_hip_ctx alac_hip_ctx;

/* What InitializeEncoder derives from AudioFormatDescription (codec/ALACEncoder.cu:1457-1479)
 * plus SetFrameSize (codec/ALACEncoder.h:47). */
typedef struct alac_hip_format {
    uint32_t frame_size;   /* sample-frames per packet; kALACDefaultFramesPerPacket = 4096 */
    uint32_t bit_depth;    /* 16, 20, 24 or 32 (mFormatFlags 1..4) */
    uint32_t num_channels; /* 1 (ID_SCE), 2 (ID_CPE) or 3..8: the element sequence of sChannelMaps
                            * (codec/ALACEncoder.cu:97-107), e.g. 6 = SCE CPE CPE SCE */
    uint32_t sample_rate;  /* only carried into the magic cookie */
} alac_hip_format;

/* int16 values of coefficient state per segment for this format (64 x elements per packet). */
uint32_t alac_hip_state_int16(const alac_hip_format *fmt);

/* ---- context ---------------------------------------------------------------------------- */

/* Number of HIP devices visible; < 0 on failure. */
int32_t alac_hip_device_count(void);

/* Create a context bound to `device`.  `stream` is a hipStream_t to enqueue on (NULL = a stream
 * the context creates and owns).  Replaces the implicit default-stream/device-0 use of the fork
 * (codec/ALACEncoder.cu:1494-1512). */
int32_t alac_hip_create(alac_hip_ctx **out_ctx, int32_t device, void *stream);
void alac_hip_destroy(alac_hip_ctx *ctx);
/* Block until everything enqueued on the context's stream has completed
 * (the cudaDeviceSynchronize of codec/ALACEncoder.cu:1448).  Returns kALAC_MemFullError if, in any call since the last
 * synchronize, a consumer wave of an in-launch producer/consumer hand-off gave up waiting (a preempted or lost producer):
 * the outputs of those calls are then invalid (the decoder also marks the packets concerned kALAC_ParamError).  The
 * host-buffer entry points below return the same code themselves. */
int32_t alac_hip_synchronize(alac_hip_ctx *ctx);
/* Code-path switches of ONE context (no reference counterpart: the reference has a single path).  The library picks a
 * regime per call from the batch shape; a caller can pin one.  The ALAC_HIP_<KEY> environment variables only provide the
 * defaults a context is created with.  Keys (value range; -1 = automatic):
 *   "thru" (-1/0/1)        encode: throughput regime — one kernel per stage, a chain's predictor and coder in one lane,
 *                          final pass per packet class; automatic above 65 536 chains
 *   "narrow" (-1/0/1)      encode: four lanes per chain instead of two; automatic (-1): up to 11 264 chains (5 632 stereo packets;
 *                          mono: 10 240), and again from 21 761 to 34 816 chains (mono: 26 112), where the two-lane workers no
 *                          longer have a SIMD each
 *   "fused" (0/1)          encode: predictor || entropy coder as producer/consumer launches (latency and tiny regimes);
 *                          0 = one plain kernel per stage ("stagewise").  Frames above 524 287 samples keep their regime
 *                          and its fused final launch; only the mixRes search in front of it runs as plain launches
 *                          (its progress word counts the rows of a pass in 16 bits), and "overlap_pos" is off with it
 *   "fold" (0/1)           latency regime: numU / numV / escape decision and the packet sizes inside the final launch
 *   "pub_every" (1/2/4/8)  latency and tiny regimes: the predictor waves of the producer/consumer launches tell their consumers
 *                          about finished residual rows every 1, 2, 4 or 8 tiles, and after every tile at the end of a pass
 *   "split_coder" (0/1)    tiny regime: the final coder of a chain on two waves
 *   "overlap_pos" (0/1)    chained tiny batches: packet position p + 1's search beside position p's final pass
 *   "fast_mode" (0/1)      ALACEncoder::SetFastMode: the search-free stereo path (EncodeStereoFast).  The first-generation
 *                          encoder has no such form: 2-channel streams run on the tap-parallel pipeline while this is 1,
 *                          whatever "encoder_lane" says
 *   "encoder_lane", "decoder_lane" (0/1)   the first-generation lane-per-chain kernels (a second, structurally different
 *                          implementation kept for differential testing)
 *   "dec_fused" (-1/0/1)   decode: entropy wave + its predictor waves in one launch; automatic up to 65 536 chains (mono: 49 152)
 *   "dec_pair" (0/1)       decode, separate launches, 16- / 20- / 24-bit stereo: the two predictor lanes of a packet un-mix and
 *                          write the PCM
 *   "dec_direct" (0/1/2)   decode, separate launches, 16-bit: the kernels read the caller's stream (dword aligned) instead of a
 *                          staged copy: 0 never, 1 (default) from 80 000 packets on (below that the swap per word on the
 *                          entropy lanes' chain costs more than the copy), 2 whenever the stream allows it
 *   "stage_taps" (0/1)     alac_hip_pc_block: tap-parallel kernel for 5..30 taps
 *   "lpc" (0/1)            encode, every entry point: independent packets whose channels may carry predictor coefficients
 *                          computed from the packet's own PCM (autocorrelation + Levinson-Durbin, orders 4 8 12 16 24 30, any
 *                          denShift <= 15, counted exactly on the GPU) wherever they code smaller than Apple's init_coefs
 *                          channel; a packet is never larger than with one segment per packet.  The segment table is
 *                          ignored (every packet is its own segment: size the workspace with num_segments = num_packets, and
 *                          pass the packet count to alac_hip_encode_regime), d_state is neither read nor written, escaped
 *                          packets stay escaped.  Mono and stereo, frame_size x channels <= 16 384; 3..8 channels, or
 *                          "fast_mode" = 1 at the same time -> kALAC_ParamError from the encode call.  NOT the reference's
 *                          bytes (decoders that follow the format decode it; orders above 8 take their generic predictor)
 *   "debug_waves" (0/1)    diagnostics, see alac_hip_debug_waves_offset
 *   "debug_lose_handoff" (0/1)  TEST switch, the one key that invalidates results by design: producers of the in-launch
 *                          hand-offs never publish, so every call fails with kALAC_MemFullError at the next synchronize
 * Every other setting except "lpc" produces the same bytes; only the kernels that run differ.  Unknown key or a value outside the
 * key's range -> kALAC_ParamError. */
int32_t alac_hip_set_option(alac_hip_ctx *ctx, const char *key, int32_t value);
int32_t alac_hip_get_option(alac_hip_ctx *ctx, const char *key, int32_t *value);
/* Diagnostics: with option "debug_waves" = 1 the fused final launch of alac_hip_encode leaves 8 dwords per workgroup at this
 * byte offset of the caller's workspace (HW_ID, XCC_ID, s_memtime at entry, at exit, HW_ID at exit, 0): where and when every
 * wave ran (tools/wave_map.py).  Batches above 4096 chains only (below, the words are the row-ready flags of chained files). */
uint64_t alac_hip_debug_waves_offset(const alac_hip_format *fmt, uint32_t num_packets, uint32_t num_segments);
/* The encode regime this context would pick for a batch of num_segments independent segments of this format (option "lpc":
 * num_segments = the packet count, every packet is its own segment there) (a static
 * string, from the launcher's own predicates): "throughput" (separate launches, 64 chains per wave), "latency"
 * (producer/consumer launches, two lanes per chain), "tiny" (four lanes per chain: chained files), "stagewise" (option
 * "fused" = 0) or "lane" (first-generation kernel).  For reporting. */
const char *alac_hip_encode_regime(alac_hip_ctx *ctx, const alac_hip_format *fmt, uint32_t num_segments);
/* Text of the last HIP/parameter error on this context ("" if none). */
const char *alac_hip_last_error(const alac_hip_ctx *ctx);
/* The stream the context enqueues on (hipStream_t as void*), for event timing by the caller. */
void *alac_hip_stream(const alac_hip_ctx *ctx);

/* ---- batch encode: replaces InitializeSampling + the per-packet Encode loop ----------------
 * (codec/ALACEncoder.cu:1385-1451, :973-1057, :290-558, :749-806, :812-963; the stage calls
 *  pc_block codec/dp_enc.c:77, dyn_comp codec/ag_enc.c:249, mixNN codec/matrix_enc.cu:101-425). */

/* Bytes of device scratch alac_hip_encode needs for this shape (option "lpc": num_segments = num_packets). */
uint64_t alac_hip_encode_workspace_bytes(const alac_hip_format *fmt, uint32_t num_packets,
                                         uint32_t num_segments);
/* Upper bound of the packed output of num_packets packets (every packet escaped + header). */
uint64_t alac_hip_encode_max_output_bytes(const alac_hip_format *fmt, uint32_t num_packets);

/*
 * Encode num_packets packets.
 *   d_pcm            packed little-endian interleaved PCM; packet p starts at byte
 *                    p * frame_size * num_channels * bytes_per_sample (convert-utility/main.cu:509)
 *   d_num_samples    [num_packets] sample-frames in each packet (<= frame_size), or NULL = all full
 *                    (the outBytes[] of InitializeSampling, in samples)
 *   d_seg_first      [num_segments + 1] first packet index of each segment (a segment = a run of
 *                    packets chained through the coefficient state), or NULL =
 *                    every packet is its own segment (state = init_coefs, codec/dp_enc.c:49-60)
 *   d_state          [elements][num_segments][ALAC_HIP_STATE_INT16] coefficient rows (elements = 1 up
 *                    to 2 channels); read as the initial state when state_in != 0, always written
 *                    with the final state when non-NULL
 *   d_out            packets written back to back (each byte-aligned, codec/ALACEncoder.cu:1039)
 *   d_packet_bytes   [num_packets] size of each packet (the *ioNumBytes of Encode)
 *   d_packet_offsets [num_packets + 1] exclusive scan of the sizes; last entry = total bytes
 * Returns ParamError for an unsupported format or a too-small workspace/output.
 */
int32_t alac_hip_encode(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_pcm,
                        const uint32_t *d_num_samples, uint32_t num_packets,
                        const uint32_t *d_seg_first, uint32_t num_segments, int16_t *d_state,
                        int32_t state_in, void *d_workspace, uint64_t workspace_bytes,
                        uint8_t *d_out, uint64_t out_capacity, uint32_t *d_packet_bytes,
                        uint64_t *d_packet_offsets);

/* The same with the caller's bound on the packets of a segment.  The pipeline runs once per packet position of the longest
 * segment, so the host has to know that length: alac_hip_encode reads d_seg_first back (one blocking copy per call) when it is
 * given a table; here max_segment_packets (> 0) is taken on trust, nothing is read back and the call stays asynchronous.  The
 * table is checked on the device (ascending, 0 .. num_packets, no segment above the bound); if it fails, the next
 * alac_hip_synchronize returns kALAC_ParamError and NOTHING has been written to d_out (offsets are all zero): every kernel
 * tests the table entry it uses against num_packets and the bound before it forms a packet index (a segment that fails has
 * no packets), and the size scan and the packer produce nothing once the check has failed — an unvalidated table can make
 * the call fail, never make it read or write out of bounds.  An over-estimate only costs idle launches.
 * max_segment_packets = 0: exactly alac_hip_encode.  (The fork's InitializeSampling has no counterpart: one file, one chain.) */
int32_t alac_hip_encode_segmented(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_pcm,
                                  const uint32_t *d_num_samples, uint32_t num_packets,
                                  const uint32_t *d_seg_first, uint32_t num_segments,
                                  uint32_t max_segment_packets, int16_t *d_state, int32_t state_in,
                                  void *d_workspace, uint64_t workspace_bytes, uint8_t *d_out,
                                  uint64_t out_capacity, uint32_t *d_packet_bytes, uint64_t *d_packet_offsets);

/* ---- batch encode from float32 PCM ------------------------------------------------------------------------------------
 * The encode-side counterpart of alac_hip_decode_float: a PyTorch caller holding a float32 [channels, frames] tensor (or a
 * WAV file's interleaved [frames, channels] floats) encodes it without quantizing, interleaving and packing it first.  No
 * reference counterpart.  The call means "quantize by the rule below, then alac_hip_encode_segmented on the result": every
 * encode option (lpc, fast_mode, the regime keys), the segment table, max_segment_packets and the state rules are those of
 * alac_hip_encode_segmented, and the bytes, sizes, offsets and final state are what it gives for the quantized PCM.
 * Asynchronous like alac_hip_encode_segmented.
 * Quantization, for bit depth b in {16, 20, 24, 32} and an input float x:
 *     r = rint(x * 2^(b-1))                 # round half to even; the product is exact (power-of-two scale)
 *     s = 0                 if x is NaN
 *         2^(b-1) - 1       if r >  2^(b-1) - 1   (+inf included)
 *         -2^(b-1)          if r < -2^(b-1)       (-inf included)
 *         (int) r           otherwise
 *     clipped(x) = x is NaN or r was outside [-2^(b-1), 2^(b-1) - 1]
 *   x = 1.0 clips to 2^(b-1) - 1 and counts as clipped; x = -1.0 is exact; -0.0 and denormals give 0.  At 32 bits the
 *   float product is exact and every finite x < 1.0 is at most 2^31 - 128, so it never clips.  A 20-bit sample goes into
 *   its 3-byte container left-justified (s << 4), as alac_hip_encode reads it.  So alac_hip_decode_float(alac_hip_encode_float
 *   (x)) == x bit for bit whenever x * 2^(b-1) is an integer in range.  (Not with the dither of
 *   alac_hip_encode_float_dither below: there the rounding is of x * 2^(b-1) + d.)
 *   d_in              float32, 4-byte aligned: sample i of channel c of packet p at
 *                     d_in[c * channel_stride + (p * frame_size + i) * frame_stride].  Planar [C, T] is (channel_stride >= T,
 *                     frame_stride = 1), interleaved [T, C] is (channel_stride = 1, frame_stride = C); both take 16-byte
 *                     vector loads when frame_size is a multiple of 4, d_in is 16-byte aligned and (planar) channel_stride
 *                     is a multiple of 4; any other layout takes one load per sample.
 *   d_num_samples     as alac_hip_encode.  Only min(num_samples[p], frame_size) frames of packet p are read: nothing between
 *                     rows, nothing behind a short last packet (a tensor of exactly T frames is safe); the staged frames
 *                     behind them are zero.
 *   d_workspace       alac_hip_encode_float_workspace_bytes bytes, 256-byte aligned: the encode workspace followed by the
 *                     staged integer PCM (the last whole 256-byte blocks of workspace_bytes hold the stage, the encoder gets
 *                     the rest).  Option lpc: size it for num_segments = num_packets, as for alac_hip_encode.
 *   d_clipped         [num_packets] count of clipped samples per packet, or NULL (not counted)
 *   the other arguments as alac_hip_encode_segmented.
 * kALAC_ParamError, checked before anything is enqueued and with nothing written: a null or misaligned d_in, frame_stride 0,
 * channel_stride 0 with more than one channel, a largest index (num_channels - 1) * channel_stride + (num_packets *
 * frame_size - 1) * frame_stride whose byte offset overflows 64 bits, a workspace too small, and whatever
 * alac_hip_encode_segmented refuses (a segment table without a bound is read back and checked first, where that call reads
 * it back).
 */
uint64_t alac_hip_encode_float_workspace_bytes(const alac_hip_format *fmt, uint32_t num_packets, uint32_t num_segments);
int32_t alac_hip_encode_float(alac_hip_ctx *ctx, const alac_hip_format *fmt, const float *d_in,
                              uint64_t channel_stride, uint64_t frame_stride,
                              const uint32_t *d_num_samples, uint32_t num_packets,
                              const uint32_t *d_seg_first, uint32_t num_segments, uint32_t max_segment_packets,
                              int16_t *d_state, int32_t state_in, void *d_workspace, uint64_t workspace_bytes,
                              uint8_t *d_out, uint64_t out_capacity, uint32_t *d_packet_bytes,
                              uint64_t *d_packet_offsets, uint32_t *d_clipped);
/* Host-buffer form (synchronous, like alac_hip_encode_host_segments, whose table rules it shares): h_in in the layout above;
 * the floats up to the last frame that h_num_samples covers are staged to the device.  h_clipped: [num_packets] or NULL. */
int32_t alac_hip_encode_float_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const float *h_in,
                                   uint64_t channel_stride, uint64_t frame_stride,
                                   const uint32_t *h_num_samples, uint32_t num_packets,
                                   const uint32_t *h_seg_first, uint32_t num_segments, int16_t *h_state,
                                   int32_t state_in, uint8_t *h_out, uint64_t out_capacity,
                                   uint32_t *h_packet_bytes, uint64_t *out_total_bytes, uint32_t *h_clipped);

/* ---- TPDF dither in front of the rounding of alac_hip_encode_float ------------------------------------------------------
 * What every tool that reduces float audio to 16 bits adds by default: triangular dither of +-1 LSB, so that the error of
 * the quantization has mean 0 and variance 1/4 LSB^2 whatever the input instead of following the signal.  The dither comes
 * from a counter-based generator: it is a pure function of (seed, channel, frame index), generated on the device in the
 * same pass that quantizes, and reproducible bit for bit on the host.  No reference counterpart.
 * The rule, for bit depth b in {16, 20, 24}, seed S (64 bits), channel c (its index in the call, 0-based), and stream
 * frame index t (64 bits) of the sample:
 *     T  = t >> 1
 *     w  = Philox4x32-10( counter = (T & 0xffffffff, T >> 32, c, 0),  key = (S & 0xffffffff, S >> 32) )   # 4 words
 *     (wa, wb) = (w[0], w[1]) if t is even, (w[2], w[3]) if t is odd       # one Philox call serves two frames
 *     k  = (int)(wa >> 8) - (int)(wb >> 8)                                  # -(2^24 - 1) .. 2^24 - 1, triangular
 *     d  = (float)k * 2^-24                                                 # exact; strictly inside (-1, 1) LSB
 *     v  = x * 2^(b-1) + d        rounded ONCE to float32  (the product is exact, so fmaf and mul-then-add agree)
 *     r  = rint(v)                                                          # then exactly the existing rule:
 *     s, clipped(x)  as alac_hip_encode_float defines them from r           # saturation, NaN -> 0 and clipped
 *   Philox4x32-10 is the generator of Salmon et al. (Random123; multipliers 0xD2511F53 / 0xCD9E8D57, key increments
 *   0x9E3779B9 / 0xBB67AE85, ten rounds).  t = origin[p] + i for sample-frame i of packet p, where origin is
 *   d_packet_origin, an optional [num_packets] uint64 table (8-byte aligned), and p * frame_size when it is NULL.  The table
 *   keeps a file's bytes the same whether it is encoded alone or as one of many in a batch (number every file's frames
 *   from 0).  Frames at or behind num_samples[p] are staged as zero as in alac_hip_encode_float: no dither there.  Because
 *   the key is the frame index and not the packet, the quantized PCM does not depend on frame_size, the layout of the
 *   input, the segment table or the encode options.  Digital silence is dithered like everything else.
 *   In float64 the sum x * 2^(b-1) + d is exact whenever |x * 2^(b-1)| < 2^29, which covers everything that does not
 *   saturate, so float32(float64(x) * 2^(b-1) + float64(d)) is the host restatement (tests/dither_ref.py).
 *   With dither on, alac_hip_decode_float(alac_hip_encode_float_dither(x)) == x no longer holds on the grid: that is the point.
 * dither == NULL or mode ALAC_HIP_DITHER_NONE: exactly alac_hip_encode_float (d_packet_origin is ignored).  The workspace is
 * that of alac_hip_encode_float_workspace_bytes.  Asynchronous like alac_hip_encode_float; *dither is read before the call
 * returns.  kALAC_ParamError, checked before anything is enqueued and with nothing written: a mode above
 * ALAC_HIP_DITHER_TPDF, reserved != 0, bit depth 32 with mode TPDF (a float32 carries nothing below a 32-bit LSB, and the
 * one-rounding rule cannot be restated in float64 there), a d_packet_origin that is not 8-byte aligned, and everything
 * alac_hip_encode_float refuses.
 */
enum { ALAC_HIP_DITHER_NONE = 0, ALAC_HIP_DITHER_TPDF = 1 };
typedef struct alac_hip_dither {
    uint32_t mode;     /* ALAC_HIP_DITHER_* */
    uint32_t reserved; /* 0 */
    uint64_t seed;
} alac_hip_dither;
int32_t alac_hip_encode_float_dither(alac_hip_ctx *ctx, const alac_hip_format *fmt, const float *d_in,
                                     uint64_t channel_stride, uint64_t frame_stride,
                                     const uint32_t *d_num_samples, uint32_t num_packets,
                                     const uint32_t *d_seg_first, uint32_t num_segments, uint32_t max_segment_packets,
                                     int16_t *d_state, int32_t state_in, void *d_workspace, uint64_t workspace_bytes,
                                     uint8_t *d_out, uint64_t out_capacity, uint32_t *d_packet_bytes,
                                     uint64_t *d_packet_offsets, uint32_t *d_clipped,
                                     const alac_hip_dither *dither, const uint64_t *d_packet_origin);
/* Host-buffer form: alac_hip_encode_float_host with the dither above; h_packet_origin: [num_packets] on the host, or NULL. */
int32_t alac_hip_encode_float_dither_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const float *h_in,
                                          uint64_t channel_stride, uint64_t frame_stride,
                                          const uint32_t *h_num_samples, uint32_t num_packets,
                                          const uint32_t *h_seg_first, uint32_t num_segments, int16_t *h_state,
                                          int32_t state_in, uint8_t *h_out, uint64_t out_capacity,
                                          uint32_t *h_packet_bytes, uint64_t *out_total_bytes, uint32_t *h_clipped,
                                          const alac_hip_dither *dither, const uint64_t *h_packet_origin);

/* ---- batch encode from integer PCM of any layout, container and depth ------------------------------------------------
 * The integer counterpart of alac_hip_encode_float: a PyTorch caller holds planar [channels, frames] int16 / int32 tensors
 * (torchaudio.load(normalize=False), soundfile.read(dtype="int32")), a 24-bit file arrives as int32, left- or right-
 * justified, and a 24-bit master is reduced to 16 bits with dither.  alac_hip_pcm_requantize converts such a source into the
 * packed interleaved PCM alac_hip_encode reads and alac_hip_verify expects (one streaming pass); alac_hip_encode_int means
 * "alac_hip_pcm_requantize into the tail of the workspace, then alac_hip_encode_segmented on the result".  No reference
 * counterpart.
 * The source, alac_hip_int_source: containers of container_bytes bytes (2: int16, 3: packed little-endian, 4: int32), of which
 * S = bits are significant.  Sample i of channel c of packet p is the container at index
 *     c * channel_stride + (p * frame_size + i) * frame_stride            (in containers)
 * exactly the indexing of alac_hip_encode_float, so planar, interleaved and transposed views all need no copy.
 *     left_justified = 1:  s = container >> (8 * container_bytes - S), arithmetic; the bits below are not part of the sample
 *     left_justified = 0:  s = the sign-extended container, expected in [-2^(S-1), 2^(S-1)); a container outside that range
 *                          is saturated to it first, and the sample counts as clipped
 * The rule, for the target depth b = fmt->bit_depth in {16, 20, 24, 32}:
 *   widening and identity, b >= S:   r = s << (b - S), exact; nothing is rounded, so dither is refused here
 *   reduction, b < S, D = S - b (4, 8, 12 or 16), in 64-bit integers:
 *     k   = (int)(wa >> 8) - (int)(wb >> 8) of the dither rule above, for (seed, channel c, stream frame t = origin[p] + i):
 *           the same Philox4x32-10 words, counters and one-call-serves-two-frames layout; without dither k = 0
 *     acc = s * 2^(24 - D) + k                                              # |acc| < 2^52
 *     q   = acc >> 24 (floor),  rem = acc & (2^24 - 1)
 *     r   = q + (rem > 2^23  or  (rem == 2^23 and q is odd))                # round half to even of acc / 2^24
 *     out = clamp(r, -2^(b-1), 2^(b-1) - 1)
 *     clipped = the container was out of range, or r was outside that interval
 *   A 20-bit result goes into its 3-byte container left-justified (out << 4), as everywhere else in the library.  Frames at
 *   or behind min(num_samples[p], frame_size) are not read; they are staged as zero, with no dither.
 *   Relation to the float rule.  Undithered and S <= 24 the result EQUALS that of alac_hip_encode_float on x = s * 2^-(S-1),
 *   samples and clip flags alike (x and x * 2^(b-1) are exact floats, and both rules round half to even).  With dither the two
 *   rules DIFFER in some samples (0.06 - 1 % of them): the float rule rounds the sum x * 2^(b-1) + d to float32 once before
 *   rint, the integer rule rounds the exact sum.  The paths are not interchangeable under dither; a stream dithered here is
 *   verified with alac_hip_pcm_requantize + alac_hip_verify, not with alac_hip_verify_float.  The error out - s / 2^D of the
 *   dithered integer rule has mean 0 and variance 1/4 LSB^2 at all six (S, b) pairs.
 * alac_hip_pcm_requantize: the conversion alone, asynchronous.
 *   d_in              the containers; 2- and 4-byte containers aligned to their size.  1 and 2 channels take vector loads
 *                     when frame_size is a multiple of 4 and base and strides are aligned: planar and interleaved int32
 *                     (16-byte aligned d_in, planar channel_stride a multiple of 4), planar and interleaved int16 (8-byte
 *                     aligned), interleaved packed 3-byte (4-byte aligned).  Everything else takes one load per sample.
 *   d_num_samples     [num_packets] or NULL (every packet frame_size frames)
 *   d_pcm_out         16-byte aligned, pcm_capacity >= num_packets * frame_size * num_channels * container bytes of b
 *   d_clipped         [num_packets] count of clipped samples per packet, or NULL
 *   dither, d_packet_origin   as alac_hip_encode_float_dither; mode TPDF only where b < S
 * alac_hip_encode_int: the arguments of alac_hip_encode_float_dither with (d_in, src) for the float pointer and its strides;
 *   the workspace is alac_hip_encode_int_workspace_bytes (the value of alac_hip_encode_float_workspace_bytes).  The encode
 *   options, the segment table, max_segment_packets and the state rules are those of alac_hip_encode_segmented, and the bytes
 *   are those of alac_hip_encode on the requantized PCM.  *src and *dither are read before the call returns.
 * kALAC_ParamError, checked before anything is enqueued and with nothing written: null d_in or src; container_bytes not 2, 3
 * or 4; bits not 16, 20, 24 or 32, or above 8 * container_bytes; reserved != 0; left_justified > 1; d_in not aligned to a 2-
 * or 4-byte container; frame_stride 0; channel_stride 0 with more than one channel; a largest index whose byte offset
 * overflows 64 bits; mode TPDF with b >= S; what alac_hip_encode_float_dither refuses in a dither struct or an origin table;
 * a workspace or output that is too small or misaligned; and everything alac_hip_encode_segmented refuses.
 */
typedef struct alac_hip_int_source {
    uint32_t container_bytes; /* 2 (int16), 3 (packed little-endian), 4 (int32) */
    uint32_t bits;            /* S: significant bits, 16 / 20 / 24 / 32, S <= 8 * container_bytes */
    uint32_t left_justified;  /* 1: sample = container >> (8*container_bytes - S), arithmetic; the bits below are not part of
                                 the sample.  0: sample = the sign-extended container, expected in [-2^(S-1), 2^(S-1)) */
    uint32_t reserved;        /* 0 */
    uint64_t channel_stride;  /* in containers */
    uint64_t frame_stride;    /* in containers */
} alac_hip_int_source;
int32_t alac_hip_pcm_requantize(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_in,
                                const alac_hip_int_source *src, const uint32_t *d_num_samples, uint32_t num_packets,
                                uint8_t *d_pcm_out, uint64_t pcm_capacity, uint32_t *d_clipped,
                                const alac_hip_dither *dither, const uint64_t *d_packet_origin);
uint64_t alac_hip_encode_int_workspace_bytes(const alac_hip_format *fmt, uint32_t num_packets, uint32_t num_segments);
int32_t alac_hip_encode_int(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *d_in,
                            const alac_hip_int_source *src, const uint32_t *d_num_samples, uint32_t num_packets,
                            const uint32_t *d_seg_first, uint32_t num_segments, uint32_t max_segment_packets,
                            int16_t *d_state, int32_t state_in, void *d_workspace, uint64_t workspace_bytes,
                            uint8_t *d_out, uint64_t out_capacity, uint32_t *d_packet_bytes,
                            uint64_t *d_packet_offsets, uint32_t *d_clipped,
                            const alac_hip_dither *dither, const uint64_t *d_packet_origin);
/* Host-buffer forms (synchronous): h_in in the layout above; only the containers up to the last frame that h_num_samples
 * covers are staged to the device (h_num_samples NULL in alac_hip_pcm_requantize_host: every packet frame_size frames).
 * alac_hip_encode_int_host shares the table rules of alac_hip_encode_host_segments. */
int32_t alac_hip_pcm_requantize_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *h_in,
                                     const alac_hip_int_source *src, const uint32_t *h_num_samples, uint32_t num_packets,
                                     uint8_t *h_pcm_out, uint64_t pcm_capacity, uint32_t *h_clipped,
                                     const alac_hip_dither *dither, const uint64_t *h_packet_origin);
int32_t alac_hip_encode_int_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *h_in,
                                 const alac_hip_int_source *src, const uint32_t *h_num_samples, uint32_t num_packets,
                                 const uint32_t *h_seg_first, uint32_t num_segments, int16_t *h_state, int32_t state_in,
                                 uint8_t *h_out, uint64_t out_capacity, uint32_t *h_packet_bytes,
                                 uint64_t *out_total_bytes, uint32_t *h_clipped,
                                 const alac_hip_dither *dither, const uint64_t *h_packet_origin);

/* Per-kernel timing with HIP events recorded on the context's stream around the three kernels of
 * alac_hip_encode (the instrumented counterpart of the dead cudaEvent timing in
 * codec/CudaAlacEncoder.cu:52-65).  begin() arms up to max_calls encode calls; end() synchronises and
 * returns the number of calls timed and the mean milliseconds of every pipeline stage. */
int32_t alac_hip_profile_begin(alac_hip_ctx *ctx, uint32_t max_calls);
/* out_stage_ms: [alac_hip_num_stages()] mean milliseconds of ONE launch of each pipeline stage
 * (alac_hip_stage_name(i)); out_launches: launches of that stage per encode call (the predictor and
 * Golomb stages run once per overlapped sub-batch). */
int32_t alac_hip_profile_end(alac_hip_ctx *ctx, uint32_t *out_calls, float *out_stage_ms,
                             uint32_t *out_launches);
uint32_t alac_hip_num_stages(void);
const char *alac_hip_stage_name(uint32_t stage);

/* 24-byte magic cookie (ALACSpecificConfig, big-endian): GetConfig/GetMagicCookie
 * (codec/ALACEncoder.cu:1082-1140) for <= 2 channels.  Host-only, no device work. */
uint32_t alac_hip_magic_cookie(const alac_hip_format *fmt, uint32_t max_frame_bytes,
                               uint32_t avg_bit_rate, uint8_t *h_cookie24);
/* GetMagicCookieSize / GetMagicCookie for any channel count (codec/ALACEncoder.cu:1097-1140): above 2
 * channels the config is followed by the 12-byte 'chan' atom header and the 12-byte
 * ALACAudioChannelLayout (48 bytes in all; the layout tag in host byte order as the fork writes it).
 * Returns the bytes written, 0 if `capacity` is too small ("no incomplete cookies", :1136-1139). */
uint32_t alac_hip_magic_cookie_size(const alac_hip_format *fmt);
uint32_t alac_hip_magic_cookie_full(const alac_hip_format *fmt, uint32_t max_frame_bytes,
                                    uint32_t avg_bit_rate, uint8_t *h_cookie, uint32_t capacity);

/* ---- batch decode: replaces ALACDecoder::Decode + fillWriteBuffer ---------------------------
 * (codec/ALACDecoder.cu:571-1002, :497-563; dyn_decomp codec/ag_dec.c:272, unpc_block
 *  codec/dp_dec.c:55, gpu_unmixNN codec/ALACDecoder.cu:193-383). */

uint64_t alac_hip_decode_workspace_bytes(const alac_hip_format *fmt, uint32_t num_packets);
/* The same for a stream of known length: packets padded with ID_FIL / ID_DSE elements (which the decoder skips,
 * codec/ALACDecoder.cu:1012-1059) can make a legal stream longer than num_packets regular packets.  alac_hip_decode
 * uses all of the workspace it is given; packets that still do not fit get status kALAC_ParamError. */
uint64_t alac_hip_decode_workspace_bytes_stream(const alac_hip_format *fmt, uint32_t num_packets,
                                                uint64_t stream_bytes);

/*
 * Decode num_packets packets (independent: coefficients travel in each packet header).
 *   h_cookie/size     magic cookie as stored in the CAF 'kuki' chunk (ALACDecoder::Init,
 *                     codec/ALACDecoder.cu:109-190; legacy 'frma'/'alac' wrappers are skipped)
 *   d_stream          packets back to back
 *   d_packet_offsets  [num_packets + 1] byte offset of each packet in d_stream
 *   d_pcm_out         packet p is written at p * frame_size * num_channels * bytes_per_sample
 *   d_num_samples_out [num_packets] decoded sample-frames per packet (outNumSamples of Decode)
 *   d_status          [num_packets] per-packet status (0 or kALAC_ParamError)
 */
int32_t alac_hip_decode(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size,
                        const uint8_t *d_stream, const uint64_t *d_packet_offsets,
                        uint32_t num_packets, void *d_workspace, uint64_t workspace_bytes,
                        uint8_t *d_pcm_out, uint32_t *d_num_samples_out, int32_t *d_status);

/* ---- batch decode to planar float32 ----------------------------------------------------------------------------------
 * alac_hip_decode with every PCM store site writing the sample as a float instead of its integer bytes: what a PyTorch
 * caller wants (a [channels, frames] float32 tensor scaled to [-1, 1), the shape torchaudio.load returns) without a second
 * pass over the output.  No reference counterpart.  Asynchronous like alac_hip_decode, same decoder options.
 *   d_out             planar float32, 4-byte aligned: sample i of channel c of packet p at
 *                     d_out[c * channel_stride + p * frame_size + i].  Channel c is the c-th sample of a frame as
 *                     alac_hip_decode interleaves it.
 *   channel_stride    floats between two channels' rows: at least num_packets * frame_size
 *   d_workspace       exactly alac_hip_decode_workspace_bytes_stream bytes suffice (there is no PCM plane), 256-byte aligned
 *   d_num_samples_out, d_status: as alac_hip_decode
 * Value: (float)s * 2^-(bit_depth - 1), s the decoded sample sign-extended at the stream's own depth (a 20-bit sample is
 * scaled by 2^-19, not taken from its left-justified 3-byte container).  The conversion rounds to nearest even and the scale
 * is a power of two, so 16-, 20- and 24-bit samples are exact and -2^(bit_depth - 1) gives -1.0.  32-bit samples round to
 * 24 significant bits: full-scale positive ones (2^31 - 64 and up) give 1.0.
 * Written are exactly the samples alac_hip_decode writes bytes for: num_samples frames of every decoded packet, 0.0 where
 * decode writes zero samples, nothing behind a short packet's frames and nothing between num_packets * frame_size and
 * channel_stride.  A failed in-launch hand-off is reported like decode's (kALAC_MemFullError at the next synchronize).
 * kALAC_ParamError, with nothing written, for a null or misaligned d_out, a channel_stride below num_packets * frame_size or
 * one whose channel_stride * num_channels * 4 bytes overflow, and whatever alac_hip_decode refuses.
 */
int32_t alac_hip_decode_float(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size,
                              const uint8_t *d_stream, const uint64_t *d_packet_offsets, uint32_t num_packets,
                              void *d_workspace, uint64_t workspace_bytes,
                              float *d_out, uint64_t channel_stride,
                              uint32_t *d_num_samples_out, int32_t *d_status);
/* Host-buffer form (synchronous, like alac_hip_decode_host): packets back to back with sizes h_packet_bytes; h_out in the
 * layout above, rows channel_stride floats apart; samples decode does not write come back as 0.0, the gap behind each row
 * is left as it was. */
int32_t alac_hip_decode_float_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size,
                                   const uint8_t *h_stream, const uint32_t *h_packet_bytes, uint32_t num_packets,
                                   float *h_out, uint64_t channel_stride,
                                   uint32_t *h_num_samples_out, int32_t *h_status);

/* ---- batch decode to integer PCM of any layout and container ------------------------------------------------------------
 * The decode counterpart of alac_hip_encode_int: alac_hip_decode with every PCM store site writing the decoded sample into
 * an integer container of the caller's layout, what a PyTorch caller wants (an int32 or int16 [channels, frames] tensor, the
 * shape torchaudio.load(normalize=False) and soundfile.read(dtype="int32") return), a writer of a 24-in-32 file, or a
 * caller who must keep 32-bit streams exact (alac_hip_decode_float rounds those to 24 significant bits), without a second
 * pass over the output.  No reference counterpart.  Asynchronous like alac_hip_decode, same decoder options.
 * The destination is an alac_hip_int_source read as a destination (alac_hip_int_dest): containers of container_bytes bytes
 * (2: int16, 3: packed little-endian, 4: int32), of which S = bits are significant.  Sample i of channel c of packet p goes to
 * the container at index
 *     c * channel_stride + (p * frame_size + i) * frame_stride            (in containers)
 * Channel c is the c-th sample of a frame as alac_hip_decode interleaves it.
 * The rule, for D = the stream's bit depth (from the cookie) and s = the decoded sample as alac_hip_decode stores it (its low
 * D bits, sign-extended: the wrap alac_hip_decode_float applies to damaged packets):
 *     left_justified = 1:  container = s << (8 * container_bytes - D)
 *     left_justified = 0:  container = s << (S - D), sign-extended into the container
 *   D <= S <= 8 * container_bytes.  There is no rounding, no dither and no reduction: S < D is refused, and a caller who wants
 *   fewer bits composes alac_hip_decode with alac_hip_pcm_requantize.  The rule is the inverse of the source rule of
 *   alac_hip_pcm_requantize: requantizing the output with the same descriptor at depth D gives alac_hip_decode's bytes, with
 *   zero samples clipped.  The descriptor {container_bytes = the stream's own bytes per sample, bits = D, left_justified = 1,
 *   channel_stride = 1, frame_stride = num_channels} reproduces alac_hip_decode's output byte for byte.
 * Written are exactly the samples alac_hip_decode writes bytes for: num_samples frames of every decoded packet, a zero
 * container where decode writes zero samples, nothing behind a short packet's frames and no byte outside the addressed
 * containers (a packed 3-byte container is written as its three bytes).  Where frame_stride is 1, four consecutive frames of
 * int32 or int16 containers go out as one 16- or 8-byte store; every other layout takes one store per sample.
 *   d_out             the containers; 2- and 4-byte containers aligned to their size
 *   d_workspace       exactly alac_hip_decode_workspace_bytes_stream bytes suffice (there is no PCM plane), 256-byte aligned
 *   d_num_samples_out, d_status, the hand-off error: as alac_hip_decode.  *dst is read before the call returns.
 * kALAC_ParamError, checked before anything is enqueued and with nothing written: everything alac_hip_decode refuses; null
 * d_out or dst; container_bytes not 2, 3 or 4; bits not 16, 20, 24 or 32, above 8 * container_bytes or below D;
 * left_justified > 1; reserved != 0; d_out not aligned to a 2- or 4-byte container; a largest index whose byte offset
 * overflows 64 bits; and a layout in which two samples can share a container.  With T = num_packets * frame_size and C
 * channels, exactly two families of layouts are accepted:
 *     frame_stride >= 1 and channel_stride >= T * frame_stride      (frames inner; planar is frame_stride = 1)
 *     channel_stride >= 1 and frame_stride >= C * channel_stride    (channels inner; interleaved is channel_stride = 1,
 *                                                                    frame_stride = C)
 *   With one channel only frame_stride >= 1 is required.
 */
typedef alac_hip_int_source alac_hip_int_dest;
int32_t alac_hip_decode_int(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size,
                            const uint8_t *d_stream, const uint64_t *d_packet_offsets, uint32_t num_packets,
                            void *d_workspace, uint64_t workspace_bytes,
                            void *d_out, const alac_hip_int_dest *dst,
                            uint32_t *d_num_samples_out, int32_t *d_status);
/* Host-buffer form (synchronous, like alac_hip_decode_float_host): h_out in the layout above; containers decode does not
 * write come back as zero, the bytes between containers are left as they were. */
int32_t alac_hip_decode_int_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size,
                                 const uint8_t *h_stream, const uint32_t *h_packet_bytes, uint32_t num_packets,
                                 void *h_out, const alac_hip_int_dest *dst,
                                 uint32_t *h_num_samples_out, int32_t *h_status);

/* ---- batch verify: decode and compare with the PCM the stream was encoded from, on the device ----------------------
 * What a caller of ALACDecoder::Decode (codec/ALACDecoder.cu:571-1002) does by hand before trusting an encode — decode, then
 * compare the output of fillWriteBuffer (:497-563) with the source — without writing the decoded PCM anywhere: every kernel
 * that stores PCM in alac_hip_decode loads the expected bytes at that place instead, with a load as wide as the store, and
 * compares.  That holds on every decoder path (fused and separate launches, pair lanes, direct reads, uncompressed packets,
 * the per-element rounds of 3..8 channels, the lane decoder and its fallback for other element sequences), so the answer is
 * the one "alac_hip_decode, then compare on the host" gives, and the workspace has no PCM plane.  No reference counterpart.
 *
 * Bytes of device scratch alac_hip_verify needs (stream_bytes as in alac_hip_decode_workspace_bytes_stream, 0 = every
 * packet at its largest regular size). */
uint64_t alac_hip_verify_workspace_bytes_stream(const alac_hip_format *fmt, uint32_t num_packets, uint64_t stream_bytes);

/*
 * Verify num_packets packets against the PCM they should decode to.  Asynchronous like alac_hip_decode, same decoder options.
 *   h_cookie/size          d_stream, d_packet_offsets: as alac_hip_decode
 *   d_pcm_expected         the expected PCM in the layout alac_hip_decode writes: packet p at
 *                          p * frame_size * num_channels * bytes_per_sample, 20-bit samples in 3-byte containers
 *                          (left-justified, as gpu_unmix20 writes them, codec/ALACDecoder.cu:225-280); dword aligned
 *   d_num_samples_expected [num_packets] expected sample-frames per packet, or NULL = every packet frame_size frames
 *   d_workspace            alac_hip_verify_workspace_bytes_stream bytes, 256-byte aligned
 *   d_first_mismatch       [num_packets] out: the lowest sample-frame index at which any channel differs; 0xFFFFFFFF when the
 *                          packet decodes with status 0, has the expected frame count and matches every frame.  Frame counts
 *                          that differ: min(decoded, expected) unless an earlier frame differs.  An undecodable packet: 0.
 *                          Frames behind a packet's expected count are not compared.
 *   d_status               [num_packets] out: per-packet status as alac_hip_decode reports it (0 or kALAC_ParamError)
 *   d_bad_packets          [1] out: the number of packets whose d_first_mismatch is not 0xFFFFFFFF (one word to read back)
 * The return value reports parameter and HIP errors only: a mismatch is data, not an error.
 */
int32_t alac_hip_verify(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *d_stream,
                        const uint64_t *d_packet_offsets, uint32_t num_packets, const uint8_t *d_pcm_expected,
                        const uint32_t *d_num_samples_expected, void *d_workspace, uint64_t workspace_bytes,
                        uint32_t *d_first_mismatch, int32_t *d_status, uint32_t *d_bad_packets);

/* Host-buffer form (synchronous, like alac_hip_decode_host): packets back to back with sizes h_packet_bytes; the expected
 * PCM packed as above; h_num_samples_expected, h_first_mismatch and h_status may be NULL.  Returns the number of packets that
 * failed (>= 0), or a negative status for a parameter / HIP error. */
int32_t alac_hip_verify_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *h_stream,
                             const uint32_t *h_packet_bytes, uint32_t num_packets, const uint8_t *h_pcm_expected,
                             const uint32_t *h_num_samples_expected, uint32_t *h_first_mismatch, int32_t *h_status);

/* ---- batch verify against a float32 source: what alac_hip_encode_float / _dither wrote, checked on the device -------
 * A caller who encodes from float32 has no integer PCM to hand alac_hip_verify: a rounding, a saturation, a NaN rule and
 * optionally a dither stand between the source and the stream.  This call decodes the stream and, at every place
 * alac_hip_decode would store sample i of channel c of packet p, loads
 *     x = d_in[c * channel_stride + (p * frame_size + i) * frame_stride],
 * computes the sample the float encode path stages for it — the rule of alac_hip_encode_float, or that of
 * alac_hip_encode_float_dither with t = origin[p] + i when dither has mode ALAC_HIP_DITHER_TPDF (origin = d_packet_origin,
 * p * frame_size where it is NULL) — at the stream's own bit depth (from the cookie), and compares it with the decoded
 * sample sign-extended at that depth.  The rule is the same device code the encode path runs, on every decoder path
 * alac_hip_verify covers.  Nothing is written but the outputs below; the workspace is
 * alac_hip_verify_workspace_bytes_stream (no PCM plane, no staged integer copy).  No reference counterpart.
 *   h_cookie/size, d_stream, d_packet_offsets, d_workspace: as alac_hip_verify
 *   d_in, channel_stride, frame_stride: the float32 source as alac_hip_encode_float reads it (any strides, 4-byte aligned)
 *   d_num_samples_expected [num_packets] expected sample-frames per packet, or NULL = every packet frame_size frames
 *   dither, d_packet_origin: as alac_hip_encode_float_dither; dither == NULL or mode ALAC_HIP_DITHER_NONE ignores the
 *                          origin table.  *dither is read before the call returns.
 *   d_first_mismatch, d_status, d_bad_packets: exactly alac_hip_verify's (lowest differing frame in any channel; 0xFFFFFFFF
 *                          clean; 0 undecodable; min(decoded, expected) when the counts differ and no earlier frame does)
 * Only frames i < min(expected[p], frame_size) of packet p are ever loaded from d_in (expected NULL: all frame_size),
 * whatever a damaged or foreign packet claims to contain: a tensor of exactly T frames is safe, as it is for
 * alac_hip_encode_float.  Every store site clamps by the expected count before it forms an address.
 * Asynchronous like alac_hip_verify, same decoder options, same hand-off error.  A mismatch is data, not an error.
 * kALAC_ParamError, checked before anything is enqueued and with nothing written: everything alac_hip_verify refuses; d_in
 * null or not 4-byte aligned, frame_stride 0, channel_stride 0 with more than one channel, the largest index overflowing
 * 64 bits (the checks of alac_hip_encode_float); a dither mode above ALAC_HIP_DITHER_TPDF, reserved != 0, mode TPDF on a
 * 32-bit stream, a d_packet_origin that is not 8-byte aligned.
 */
int32_t alac_hip_verify_float(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *d_stream,
                              const uint64_t *d_packet_offsets, uint32_t num_packets, const float *d_in,
                              uint64_t channel_stride, uint64_t frame_stride, const uint32_t *d_num_samples_expected,
                              const alac_hip_dither *dither, const uint64_t *d_packet_origin, void *d_workspace,
                              uint64_t workspace_bytes, uint32_t *d_first_mismatch, int32_t *d_status,
                              uint32_t *d_bad_packets);
/* Host-buffer form (synchronous, like alac_hip_verify_host): returns the number of packets that failed (>= 0), or a
 * negative status.  Stages only the floats the call may read: up to the last frame an expected count covers. */
int32_t alac_hip_verify_float_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size, const uint8_t *h_stream,
                                   const uint32_t *h_packet_bytes, uint32_t num_packets, const float *h_in,
                                   uint64_t channel_stride, uint64_t frame_stride, const uint32_t *h_num_samples_expected,
                                   const alac_hip_dither *dither, const uint64_t *h_packet_origin,
                                   uint32_t *h_first_mismatch, int32_t *h_status);

/* ---- probe float32 PCM for its lossless bit depth ------------------------------------------------------------------------
 * A float tensor is very often integer PCM in disguise (a 16-bit file loaded as float, the output of alac_hip_decode_float).
 * This call finds, per segment of frames, what alac_hip_float_report_depth needs to name the smallest depth in
 * {16, 20, 24, 32} at which alac_hip_encode_float is exactly lossless: one streaming pass over the floats that writes
 * nothing but the reports.  No reference counterpart.
 * The rule, on the bit pattern of a float32 x with biased exponent field E and mantissa field M:
 *     sig = M,             lsb = -149       if E == 0          (zero and denormals)
 *     sig = M | 0x800000,  lsb = E - 150    otherwise
 *     need(x) = 0                                   if sig == 0        (+0.0 and -0.0)
 *               max(0, 1 - (lsb + ctz(sig)))        if x is finite     (1 for -1.0, 2 for 0.5, 16 for 2^-15, 150 for the
 *                                                                       smallest denormal)
 *   x * 2^(b-1) is an integer exactly when need(x) <= b.  A set of samples encodes losslessly at depth b when no sample is
 *   NaN, no sample has x >= 1.0 or x < -1.0 (infinities count here) and max need <= b (being on the grid and below 1.0 gives
 *   the upper bound 1 - 2^-(b-1)).  Then alac_hip_decode_float(alac_hip_encode_float(x)) == x as floats: bit for bit, but
 *   that -0.0 comes back as +0.0.
 *   d_in, channel_stride, frame_stride: float32, 4-byte aligned, sample of channel c and frame t at
 *                     d_in[c * channel_stride + t * frame_stride], exactly as alac_hip_encode_float indexes it (t = p *
 *                     frame_size + i).  The same three layouts: planar and interleaved stereo take 16-byte loads when d_in is
 *                     16-byte aligned (planar: and channel_stride is a multiple of 4), 1 or 2 channels; anything else takes
 *                     one load per sample.
 *   h_seg_first_frame HOST array [num_segments + 1] of ascending frame indices, the last one <= total_frames; segment s
 *                     covers all channels of frames [first[s], first[s+1]) (it may be empty).  NULL (num_segments 1): one
 *                     segment [0, total_frames).  Read and validated before the call returns, as *dither is: it is copied
 *                     out on the host, so the caller may reuse it at once whether it is pageable or pinned memory (a call
 *                     that finds the previous call's table still on its way to the device waits for that upload).  Frames
 *                     outside every segment are not read.
 *   d_workspace       alac_hip_float_probe_workspace_bytes(num_segments) bytes, 8-byte aligned: holds the uploaded table
 *   d_reports         [num_segments] alac_hip_float_report, 8-byte aligned.  Every word is written by every call (a second
 *                     call into the same buffer does not accumulate onto the first).
 * Asynchronous on the context's stream.  kALAC_ParamError, with nothing enqueued and nothing written: a null or misaligned
 * d_in, d_reports or (with a table) d_workspace, num_channels outside 1..8, frame_stride 0, channel_stride 0 with more than
 * one channel, a largest index (num_channels - 1) * channel_stride + (total_frames - 1) * frame_stride whose byte offset
 * overflows 64 bits, num_segments 0 (or not 1 without a table), a table that is not ascending or ends behind total_frames,
 * a workspace too small.
 */
typedef struct alac_hip_float_report { /* one per segment, 32 bytes */
    uint64_t over_range;  /* samples with x >= 1.0 or x < -1.0, infinities included */
    uint64_t nan;         /* NaN samples */
    uint32_t need_bits;   /* max need(x) over the finite samples; 0 for an empty or all-zero segment */
    uint32_t peak_bits;   /* bit pattern of max |x| over the non-NaN samples (+inf possible), 0 if none */
    uint32_t reserved[2]; /* written as 0 */
} alac_hip_float_report;
uint64_t alac_hip_float_probe_workspace_bytes(uint32_t num_segments);
int32_t alac_hip_float_probe(alac_hip_ctx *ctx, const float *d_in, uint32_t num_channels, uint64_t channel_stride,
                             uint64_t frame_stride, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                             uint32_t num_segments, void *d_workspace, uint64_t workspace_bytes,
                             alac_hip_float_report *d_reports);
/* Host-buffer form (synchronous): h_in in the layout above; the floats up to the last frame of the last segment are staged
 * to the device, the reports come back in h_reports [num_segments]. */
int32_t alac_hip_float_probe_host(alac_hip_ctx *ctx, const float *h_in, uint32_t num_channels, uint64_t channel_stride,
                                  uint64_t frame_stride, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                  uint32_t num_segments, alac_hip_float_report *h_reports);
/* Host only: the smallest depth of 16, 20, 24, 32 at which the report's samples encode losslessly (an empty or all-zero
 * segment: 16); 0 when none does (nan != 0, over_range != 0 or need_bits > 32) or r is NULL. */
uint32_t alac_hip_float_report_depth(const alac_hip_float_report *r);

/* ---- probe integer PCM for its lossless bit depth -------------------------------------------------------------------------
 * ALAC has no wasted-bits field: 16-bit audio delivered in 24-bit containers pays for the zero byte in every packet, and the
 * only remedy is to encode the stream at the depth its samples really have.  This call finds, per segment of frames, what
 * alac_hip_int_report_depth needs to name the smallest depth in {16, 20, 24, 32} to which alac_hip_pcm_requantize /
 * alac_hip_encode_int reduce the source without rounding or saturating anything: one streaming pass over the containers that
 * writes nothing but the reports.  The integer counterpart of alac_hip_float_probe.  No reference counterpart.
 * The source is an alac_hip_int_source, read exactly as alac_hip_pcm_requantize reads it; the container of channel c and
 * frame t is at index c * channel_stride + t * frame_stride (alac_hip_float_probe's indexing, t = p * frame_size + i: there is
 * no packet structure).  The rule, per sign-extended container v, with S = bits and P = 8 * container_bytes - S:
 *     left_justified = 1:  s = v >> P (arithmetic),  pad = v & (2^P - 1)
 *     left_justified = 0:  s = clamp(v, -2^(S-1), 2^(S-1) - 1),  pad = 0;  the container is out of range when v != s
 *     need(s) = 0                  if s == 0
 *               S - ctz(s)         otherwise          (1 for -2^(S-1), S for an odd sample)
 *   s = r << (S - b) for an integer r exactly when need(s) <= b, so alac_hip_pcm_requantize to a depth b < S has remainder 0
 *   and rounds nothing (and b >= S is exact anyway).  For S <= 24 need(s) is alac_hip_float_probe's need(x) on
 *   x = s * 2^-(S-1); s = -2^(S-1) gives 1, as -1.0 does.
 *   d_in, src         as in alac_hip_pcm_requantize.  The same vector layouts for 1 and 2 channels: planar and interleaved
 *                     int32 with 16-byte loads (16-byte aligned d_in, planar channel_stride a multiple of 4), planar and
 *                     interleaved int16 with 8-byte loads (8-byte aligned), interleaved and mono packed 3-byte with 4-byte
 *                     loads (4-byte aligned).  Everything else takes one load per sample.
 *   h_seg_first_frame, d_workspace (alac_hip_int_probe_workspace_bytes), d_reports: as in alac_hip_float_probe, table
 *                     semantics included (ascending, may start behind frame 0 and end before total_frames, empty segments
 *                     allowed, copied out before the call returns, NULL with num_segments 1: all frames).  Frames outside
 *                     every segment are not read.  Every word of every report is written by every call.
 * Asynchronous on the context's stream.  kALAC_ParamError, with nothing enqueued and nothing written: everything
 * alac_hip_pcm_requantize refuses in a source (null d_in or src; container_bytes not 2, 3 or 4; bits not 16, 20, 24 or 32, or
 * above 8 * container_bytes; reserved != 0; left_justified > 1; d_in not aligned to a 2- or 4-byte container; frame_stride 0;
 * channel_stride 0 with more than one channel; a largest index whose byte offset overflows 64 bits) and everything
 * alac_hip_float_probe refuses in num_channels (outside 1..8), the table, the workspace and d_reports.
 */
typedef struct alac_hip_int_report { /* one per segment, 32 bytes */
    uint64_t out_of_range;     /* right-justified containers outside [-2^(S-1), 2^(S-1)); 0 when left-justified */
    uint64_t differing_frames; /* frames in which some channel's s differs from channel 0's; 0 for one channel.  0 on a stereo
                                  segment: dual mono */
    uint32_t need_bits;        /* max need(s); 0 for an empty or all-zero segment */
    uint32_t peak;             /* max |s| after saturation (up to 2^(S-1)) */
    uint32_t pad_bits;         /* OR of pad over the segment (left-justified); 0 when right-justified */
    uint32_t reserved;         /* written as 0 */
} alac_hip_int_report;
uint64_t alac_hip_int_probe_workspace_bytes(uint32_t num_segments);
int32_t alac_hip_int_probe(alac_hip_ctx *ctx, const void *d_in, const alac_hip_int_source *src, uint32_t num_channels,
                           uint64_t total_frames, const uint64_t *h_seg_first_frame, uint32_t num_segments,
                           void *d_workspace, uint64_t workspace_bytes, alac_hip_int_report *d_reports);
/* Host-buffer form (synchronous): h_in in the layout above; only the containers up to the last frame of the last segment are
 * staged to the device, the reports come back in h_reports [num_segments]. */
int32_t alac_hip_int_probe_host(alac_hip_ctx *ctx, const void *h_in, const alac_hip_int_source *src, uint32_t num_channels,
                                uint64_t total_frames, const uint64_t *h_seg_first_frame, uint32_t num_segments,
                                alac_hip_int_report *h_reports);
/* Host only: the smallest depth of 16, 20, 24, 32 that is >= need_bits (an empty or all-zero segment: 16); 0 when r is NULL,
 * out_of_range != 0 or pad_bits != 0 (the declared S loses bits, or the encode would saturate). */
uint32_t alac_hip_int_report_depth(const alac_hip_int_report *r);

/* ---- CRC-32 of PCM: the fingerprint of a decode, computed where the PCM lies -----------------------------------------------
 * ALAC carries no digest of its PCM.  This call gives one for PCM in device memory — the output of alac_hip_decode — so that
 * only the digests cross the bus: per range of bytes, the CRC-32 that zlib's crc32() gives (polynomial 0xEDB88320 reflected,
 * initial value and final XOR 0xFFFFFFFF), which is what rippers and players print for the raw PCM of a track.  One streaming
 * pass that writes nothing but the digests.  No reference counterpart.
 * The rule, in GF(2)[x] / P on reflected 32-bit words (P = 0xEDB88320; bit 31 of a word is x^0, x^8 is 0x00800000; * is the
 * product of two words mod P), with pure(A) the register after the bytes A with initial value 0 and no final XOR:
 *     pure(A || B)   = pure(A) * x^(8|B|)  ^  pure(B)
 *     crc32(A)       = pure(A)  ^  0xFFFFFFFF * x^(8|A|)  ^  0xFFFFFFFF
 *     crc32(A || B)  = crc32(A) * x^(8|B|)  ^  crc32(B)          (alac_hip_crc32_combine; zlib's crc32_combine)
 *   crc32 of no bytes is 0, of 4 zero bytes 0x2144df1c, of 8 zero bytes 0x6522df69: the length counts even for zeros.
 *   pure() is linear, so the pieces of a range are hashed independently, each is moved to the range's end by a power of x,
 *   and they are joined with XOR: the result is the same bits whatever the grid and the scheduling.
 *   d_pcm, total_bytes the bytes, any alignment (d_pcm may be NULL when total_bytes is 0)
 *   h_ranges          HOST array of num_ranges pairs {offset, length} (uint64 each), ascending and non-overlapping:
 *                     offset[i] + length[i] <= offset[i + 1], the last end <= total_bytes.  Gaps, empty ranges and any byte
 *                     alignment are allowed.  NULL (num_ranges 1): the one range [0, total_bytes).  Read and validated
 *                     before the call returns and copied out on the host, as alac_hip_float_probe's table is: the caller
 *                     may reuse it at once.  Bytes outside every range are not read.
 *   d_workspace       alac_hip_pcm_crc32_workspace_bytes(num_ranges) bytes, 8-byte aligned: holds the uploaded table (not
 *                     looked at without a table)
 *   d_digests         [num_ranges] alac_hip_pcm_digest, 8-byte aligned.  Every field is written by every call (a second call
 *                     into the same buffer does not accumulate onto the first).  crc32 of an empty range is 0.
 * Asynchronous on the context's stream.  kALAC_ParamError, with nothing enqueued and nothing written: a null or misaligned
 * d_digests, a null d_pcm with total_bytes > 0, with a table a null or misaligned d_workspace or one too small,
 * num_ranges 0 (or not 1 without a table), a table that is not ascending, overlaps, has an end that overflows 64 bits or
 * ends behind total_bytes.
 */
typedef struct alac_hip_pcm_digest { /* one per range, 16 bytes */
    uint64_t bytes;    /* the range's length */
    uint32_t crc32;    /* zlib.crc32 of the range's bytes */
    uint32_t reserved; /* written as 0 */
} alac_hip_pcm_digest;
uint64_t alac_hip_pcm_crc32_workspace_bytes(uint32_t num_ranges);
int32_t alac_hip_pcm_crc32(alac_hip_ctx *ctx, const void *d_pcm, uint64_t total_bytes, const uint64_t *h_ranges,
                           uint32_t num_ranges, void *d_workspace, uint64_t workspace_bytes, alac_hip_pcm_digest *d_digests);
/* Host-buffer form (synchronous): the bytes up to the last range's end are staged to the device, the digests come back in
 * h_digests [num_ranges]. */
int32_t alac_hip_pcm_crc32_host(alac_hip_ctx *ctx, const void *h_pcm, uint64_t total_bytes, const uint64_t *h_ranges,
                                uint32_t num_ranges, alac_hip_pcm_digest *h_digests);
/* Host only, no context: crc32(A || B) from crc_a = crc32(A), crc_b = crc32(B) and len_b = |B| — the digests of consecutive
 * pieces (a long file decoded in chunks) joined without touching the PCM again. */
uint32_t alac_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* ---- loudness of PCM: ITU-R BS.1770 energies and the sample peak, computed where the PCM lies --------------------------------
 * ReplayGain 2.0, EBU R128 and Sound Check are all BS.1770 integrated loudness plus a peak.  This call gives, for PCM in device
 * memory — the output of alac_hip_decode, alac_hip_decode_int or alac_hip_decode_float, or a source in front of an encode —
 * the K-weighted energy of every 100 ms of every channel and the peak, per segment of frames, so that only those rows cross
 * the bus; alac_hip_loudness_integrated gates them on the host.  No reference counterpart.
 * The rule.
 *   Sample value.  Integer source (alac_hip_int_source, read exactly as alac_hip_int_probe reads it): x = s * 2^-(S-1) in double,
 *     s the sample after justification and saturation; exact for every S, 32 included.  Float source, indexed as
 *     alac_hip_float_probe indexes it: x = (double)f.  A non-finite float (NaN, +inf, -inf) is read as 0.0 and counted.
 *   Filter.  Two biquads in double, run per channel from zero state at the first frame of each segment, each in the
 *     transposed direct form II (the recurrence of scipy.signal.lfilter):
 *         y = b0 x + s1;   s1 = b1 x - a1 y + s2;   s2 = b2 x - a2 y
 *     with every product-and-sum of it one fused multiply-add (y = fma(b0, x, s1); s1 = fma(b1, x, fma(-a1, y, s2));
 *     s2 = fma(b2, x, -(a2 y))), on the device and on the host alike,
 *     the shelf first, the high-pass on its output.  The coefficients for the sample rate fs are the closed forms libebur128
 *     and ffmpeg use:
 *       shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196
 *                  K = tan(pi f0 / fs), Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2
 *                  b = [(Vh + Vb K/Q + K^2), 2 (K^2 - Vh), (Vh - Vb K/Q + K^2)] / a0
 *                  a1 = 2 (K^2 - 1) / a0, a2 = (1 - K/Q + K^2) / a0
 *       high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773
 *                  b = [1, -2, 1], a1 and a2 as above from its own K
 *     At 48 kHz these are the table of BS.1770-4 to 9e-16.  fs must be a multiple of 10 in [8 000, 384 000].
 *   Energies.  hop = fs / 10 frames (100 ms).  Segment s of n frames has floor(n / hop) rows; row k, channel c holds the sum
 *     of y^2 over frames [k * hop, (k + 1) * hop) of the segment, y the filtered signal.  Frames behind the last whole hop
 *     feed the peak only.  Rows of all segments lie back to back: d_energy[(first_block[s] + k) * num_channels + c].
 *   Report.  One alac_hip_loudness_report per segment.  peak is the maximum of |x| over every frame and channel of the
 *     segment, unfiltered (the sample peak; 0 for an empty segment); nonfinite counts the non-finite floats.
 *   The device cuts a segment into chunks of L frames, L a divisor of hop and a function of fs alone, filters every chunk from
 *   zero state, carries the true states over the chunks (s' = M s + z, M the zero-input map over L frames) and filters again;
 *   the y^2 of a chunk are summed in frame order and the chunks of a hop in ascending order.  Chunking and summation order
 *   depend on the segment's own frames only: rows and reports are the same bits whatever the other segments of the call and
 *   wherever the segment lies in the buffer.  They differ from one sequential pass by rounding only (about 1e-10 relative).
 *   Integrated loudness (alac_hip_loudness_integrated, host only, no context), over num_blocks rows of one segment:
 *     gating block j covers rows j .. j+3, z_c = sum / (4 * hop);  l_j = -0.691 + 10 log10 sum_c G_c z_cj
 *     the absolute gate is -70; the relative gate lies 10 LU under the loudness of the mean over the absolutely gated blocks;
 *     the result is the loudness of the mean over the blocks that pass both gates (l_j above each gate), summed in ascending
 *     order; -HUGE_VAL when no block passes or there are fewer than 4 rows.
 *     weights == NULL takes BS.1770's weights in the channel order of the stream's ALAC layout tag (ALACAudioTypes.h:103-110):
 *       1, 2, 3 (C L R), 4 (C L R Cs)   all 1
 *       5  C L R Ls Rs                  1 1 1 1.41 1.41
 *       6  C L R Ls Rs LFE              1 1 1 1.41 1.41 0
 *       7  C L R Ls Rs Cs LFE           1 1 1 1.41 1.41 1 0
 *       8  C Lc Rc L R Ls Rs LFE        1 1 1 1 1 1.41 1.41 0
 *   d_in, src / channel_stride, frame_stride   as in alac_hip_int_probe / alac_hip_float_probe
 *   sample_rate       fs
 *   h_seg_first_frame as in alac_hip_float_probe: HOST array [num_segments + 1], ascending, may start behind frame 0 and end
 *                     before total_frames, empty segments allowed, copied out before the call returns; NULL
 *                     (num_segments 1): all frames.  Frames outside every segment are never read.
 *   d_workspace       alac_hip_loudness_workspace_bytes(sample_rate, num_channels, total_frames, num_segments) bytes, 8-byte
 *                     aligned (the call aligns its own arrays inside it), needed with and without a table: the tables, the chunks'
 *                     states and their partial sums
 *   d_energy          [energy_rows * num_channels] doubles, 8-byte aligned; energy_rows >= alac_hip_loudness_rows(...)
 *   d_reports         [num_segments] alac_hip_loudness_report, 8-byte aligned
 * Every word of every report and every row (up to the table's row count) is written by every call.  Asynchronous on the
 * context's stream.  kALAC_ParamError, with nothing enqueued and nothing written: everything alac_hip_int_probe or
 * alac_hip_float_probe refuses in the source, num_channels, the table and d_reports; a null, misaligned or too small
 * workspace; a sample rate that is not a multiple of 10 in [8 000, 384 000]; energy_rows below the table's row count (or a row
 * count above 2^32 - 1); a null or misaligned d_energy.
 */
typedef struct alac_hip_loudness_report { /* one per segment, 32 bytes */
    uint32_t first_block; /* the segment's first row of d_energy */
    uint32_t num_blocks;  /* its rows: floor(frames / hop) */
    double peak;          /* max |x| over the segment, 0 if empty */
    uint64_t nonfinite;   /* non-finite floats, read as 0.0; 0 for an integer source */
    uint64_t reserved;    /* written as 0 */
} alac_hip_loudness_report;
uint64_t alac_hip_loudness_workspace_bytes(uint32_t sample_rate, uint32_t num_channels, uint64_t total_frames,
                                           uint32_t num_segments);
int32_t alac_hip_loudness_int(alac_hip_ctx *ctx, const void *d_in, const alac_hip_int_source *src, uint32_t num_channels,
                              uint32_t sample_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                              uint32_t num_segments, void *d_workspace, uint64_t workspace_bytes, double *d_energy,
                              uint64_t energy_rows, alac_hip_loudness_report *d_reports);
int32_t alac_hip_loudness_float(alac_hip_ctx *ctx, const float *d_in, uint32_t num_channels, uint64_t channel_stride,
                                uint64_t frame_stride, uint32_t sample_rate, uint64_t total_frames,
                                const uint64_t *h_seg_first_frame, uint32_t num_segments, void *d_workspace,
                                uint64_t workspace_bytes, double *d_energy, uint64_t energy_rows,
                                alac_hip_loudness_report *d_reports);
/* Host-buffer forms (synchronous): h_in in the layout above; only the containers / floats up to the last frame of the last
 * segment are staged to the device; the rows come back in h_energy [energy_rows * num_channels] (the table's row count of
 * them is written), the reports in h_reports [num_segments]. */
int32_t alac_hip_loudness_int_host(alac_hip_ctx *ctx, const void *h_in, const alac_hip_int_source *src, uint32_t num_channels,
                                   uint32_t sample_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                   uint32_t num_segments, double *h_energy, uint64_t energy_rows,
                                   alac_hip_loudness_report *h_reports);
int32_t alac_hip_loudness_float_host(alac_hip_ctx *ctx, const float *h_in, uint32_t num_channels, uint64_t channel_stride,
                                     uint64_t frame_stride, uint32_t sample_rate, uint64_t total_frames,
                                     const uint64_t *h_seg_first_frame, uint32_t num_segments, double *h_energy,
                                     uint64_t energy_rows, alac_hip_loudness_report *h_reports);
/* Host only, no context.  alac_hip_loudness_filter: the two biquads of fs as out = {b0, b1, b2, a1, a2} of the shelf, then of
 * the high-pass; kALAC_ParamError for a bad fs or a null out.  alac_hip_loudness_rows: the rows the table's segments have in
 * all (h_seg_first_frame NULL: one segment of total_frames); 0 for a bad fs or a table alac_hip_float_probe refuses.
 * alac_hip_loudness_integrated: the rule above over h_energy [num_blocks * num_channels]; kALAC_ParamError for a null
 * h_energy (with num_blocks > 0) or out_lufs, num_channels outside 1..8 or hop 0. */
int32_t alac_hip_loudness_filter(uint32_t sample_rate, double *out);
uint64_t alac_hip_loudness_rows(uint32_t sample_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                uint32_t num_segments);
int32_t alac_hip_loudness_integrated(const double *h_energy, uint64_t num_blocks, uint32_t num_channels, uint32_t hop,
                                     const double *weights, double *out_lufs);

/* ---- true peak of PCM: ITU-R BS.1770-4 annex 2, computed where the PCM lies -----------------------------------------------------
 * The peak ReplayGain 2.0 and EBU R128 mean is the true peak: the maximum of the signal oversampled four times, which tells
 * whether applying a gain will clip (a sine at fs/4 sampled 45 degrees off its crests has a sample peak 3 dB below it).  This
 * call gives it for PCM in device memory, per segment of frames and per channel, next to the sample peak of the loudness
 * call; only a few numbers per segment cross the bus.  No reference counterpart.
 * The rule.
 *   Sample value.  Exactly that of the loudness rule above: x = s * 2^-(S-1) in double for an integer source read as
 *     alac_hip_int_probe reads it, x = (double)f for a float source indexed as alac_hip_float_probe indexes it; a non-finite
 *     float is read as 0.0 and counted.
 *   Factor.  F = 4 for fs < 96 000, F = 2 for 96 000 <= fs < 192 000, F = 1 from 192 000 up (libebur128's choice).  fs must be
 *     one the loudness call accepts: a multiple of 10 in [8 000, 384 000].
 *   Filter.  The closed form libebur128 uses, a 49-tap Hann-windowed sinc: for j = 0..48, m = j - 24,
 *         h[j] = (m == 0 ? 1 : sin(m pi / F) / (m pi / F)) * 0.5 * (1 - cos(2 pi j / 48))
 *     Tap j belongs to phase p = j mod F at index k = j div F; taps with |h[j]| < 1e-6 are dropped.  That leaves
 *       F = 4   phase 0: the single tap 1.0 at k = 6;   phases 1, 2, 3: K = 12 taps each, k = 0..11
 *       F = 2   phase 0: the single tap 1.0 at k = 12;  phase 1: K = 24 taps, k = 0..23
 *     Phase 0 is the sample itself: it is not filtered, it is the sample peak.
 *   Output samples.  For a segment of N frames and a phase p >= 1:
 *         y_p[n] = sum_k h_p[k] x[n - k]     for n in [0, N + K - 1),   x = 0 outside [0, N) of the segment
 *     accumulated from 0 with k ascending, every step one fused multiply-add, in double.  Both ends are zero-extended, so the
 *     filter's tail is flushed.  (libebur128 does not flush it and can report a true peak below the sample peak when the peak
 *     lies in the last six frames.  This rule cannot do that.)
 *   Results, per segment.  Per channel: true_peak = max(sample peak, max over p >= 1 and n of |y_p[n]|), in
 *     d_channel_peak[s * num_channels + c].  The report holds the maximum over the channels, the sample peak over the channels
 *     (the same value as alac_hip_loudness_report.peak) and the non-finite count.  F = 1: the true peak is the sample peak.  An
 *     empty segment gives 0.
 *   A segment is measured from its own frames alone: no frame outside it is read, not even as history, and the history in
 *   front of its first frame is zero whatever lies there in the buffer.  A maximum does not depend on any order, so the
 *   results are the same bits whatever the grid, the other segments of the call and the segment's place in the buffer.
 *   d_in, src / channel_stride, frame_stride, sample_rate, total_frames, h_seg_first_frame, num_segments
 *                     as in alac_hip_loudness_int / alac_hip_loudness_float
 *   d_workspace       alac_hip_true_peak_workspace_bytes(num_channels, num_segments) bytes, 8-byte aligned, needed with and
 *                     without a table: the segment tables.  It does not grow with the frame count.
 *   d_channel_peak    [num_segments * num_channels] doubles, 8-byte aligned
 *   d_reports         [num_segments] alac_hip_true_peak_report, 8-byte aligned
 * Every word of every report and of d_channel_peak is written by every call.  Asynchronous on the context's stream.
 * kALAC_ParamError, with nothing enqueued and nothing written: everything the loudness call refuses in the source,
 * num_channels, the table, the sample rate, the workspace and d_reports; a null or misaligned d_channel_peak.
 */
typedef struct alac_hip_true_peak_report { /* one per segment, 32 bytes */
    double true_peak;   /* max over the channels, 1.0 = full scale; 0 if empty */
    double peak;        /* the sample peak, as alac_hip_loudness_report.peak */
    uint64_t nonfinite; /* as there */
    uint64_t reserved;  /* written as 0 */
} alac_hip_true_peak_report;
uint64_t alac_hip_true_peak_workspace_bytes(uint32_t num_channels, uint32_t num_segments);
int32_t alac_hip_true_peak_int(alac_hip_ctx *ctx, const void *d_in, const alac_hip_int_source *src, uint32_t num_channels,
                               uint32_t sample_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                               uint32_t num_segments, void *d_workspace, uint64_t workspace_bytes, double *d_channel_peak,
                               alac_hip_true_peak_report *d_reports);
int32_t alac_hip_true_peak_float(alac_hip_ctx *ctx, const float *d_in, uint32_t num_channels, uint64_t channel_stride,
                                 uint64_t frame_stride, uint32_t sample_rate, uint64_t total_frames,
                                 const uint64_t *h_seg_first_frame, uint32_t num_segments, void *d_workspace,
                                 uint64_t workspace_bytes, double *d_channel_peak, alac_hip_true_peak_report *d_reports);
/* Host-buffer forms (synchronous): h_in in the layout above, staged as the loudness host forms stage it; the channel peaks come
 * back in h_channel_peak [num_segments * num_channels], the reports in h_reports [num_segments]. */
int32_t alac_hip_true_peak_int_host(alac_hip_ctx *ctx, const void *h_in, const alac_hip_int_source *src, uint32_t num_channels,
                                    uint32_t sample_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                    uint32_t num_segments, double *h_channel_peak, alac_hip_true_peak_report *h_reports);
int32_t alac_hip_true_peak_float_host(alac_hip_ctx *ctx, const float *h_in, uint32_t num_channels, uint64_t channel_stride,
                                      uint64_t frame_stride, uint32_t sample_rate, uint64_t total_frames,
                                      const uint64_t *h_seg_first_frame, uint32_t num_segments, double *h_channel_peak,
                                      alac_hip_true_peak_report *h_reports);
/* Host only, no context: F of fs in *out_factor, the taps per phase K (12, 24, or 0 where F = 1) in *out_taps and the
 * coefficients of phases 1 .. F-1 in out_coefs [F - 1][K] (room for 36 doubles).  The kernels take their coefficients from
 * here.  kALAC_ParamError for a bad fs or a null pointer. */
int32_t alac_hip_true_peak_filter(uint32_t sample_rate, uint32_t *out_factor, uint32_t *out_taps, double *out_coefs);

/* ---- sample-rate conversion of PCM, computed where the PCM lies ------------------------------------------------------------------
 * A 96 kHz master becomes 48 or 44.1 kHz, 44.1 kHz material becomes 48 kHz: integer or float32 PCM in device memory in, planar
 * float32 in device memory out, which is what alac_hip_encode_float takes, per segment of frames.  No reference counterpart.
 * The rule.
 *   Sample value.  Exactly that of the loudness and true-peak rules above: x = s * 2^-(S-1) in double for an integer source
 *     described by alac_hip_int_source, x = (double)f for a float32 source; a non-finite float is read as 0.0 and counted.
 *   Rates.  in_rate and out_rate are multiples of 10 in [8 000, 384 000] and are different.  With g = gcd(in_rate, out_rate),
 *     L = out_rate / g and M = in_rate / g; both must be at most 640 (every pair out of 8, 16, 22.05, 32, 44.1, 48,
 *     88.2, 96, 176.4 and 192 kHz whose ratio is at most 640/147 either way).  Anything else is kALAC_ParamError.
 *   Filter.  One quality: Z = 40 and beta = 10, K = 2 * ceil(Z * max(L, M) / L) taps per phase (80 when the rate goes up, 176
 *     for 96 -> 44.1 kHz, 350 for 192 -> 44.1 kHz).  With c = min(L, M) / M, for p in [0, L) and k in [0, K), and
 *     t = p / L + k - K / 2:
 *         h_p[k] = c * sinc(c t) * I0(beta * sqrt(max(0, 1 - (2 t / K)^2))) / I0(beta)
 *     sinc(u) = sin(pi u) / (pi u), 1 at u = 0; I0 is the modified Bessel function of the first kind and order 0 (a Kaiser
 *     window over [-K/2, K/2]).  The window is not zero at t = -K/2 (p = 0, k = 0): that tap is kept.
 *   Output.  A segment of N frames gives ceil(N * L / M) frames; output 0 sits on input frame 0, so there is no delay, and both
 *     ends are zero-extended.  For output m: n0 = (m * M) div L and p = (m * M) mod L, in 64-bit, and
 *         y[m] = (float)( sum_{k = 0}^{K - 1} h_p[k] * x[n0 + K/2 - k] ),   x = 0 outside [0, N) of the segment
 *     accumulated from 0 in double with k ascending, every step one fused multiply-add, and rounded once to float32.
 *   A segment is converted from its own frames alone: nothing outside it is read.  Every output has one order of summation, so
 *   a segment's output is the same bits whatever the grid, the other segments of the call and the segment's place in the buffer.
 *   d_in, src / channel_stride, frame_stride, total_frames, h_seg_first_frame, num_segments
 *                     as in alac_hip_loudness_int / alac_hip_loudness_float; empty segments are legal (0 frames, a zero report)
 *   d_workspace       alac_hip_resample_workspace_bytes(in_rate, out_rate, num_channels, num_segments) bytes, 16-byte aligned:
 *                     the coefficient table and the segment tables.  It does not grow with the frame count.
 *   d_out             planar float32: channel c's output frame j at d_out[c * out_channel_stride + j], the segments back to
 *                     back at the offsets alac_hip_resample_frames gives.  Floats of a row from that total on, and between the
 *                     rows, are not written.
 *   out_frames        the frames a row has room for: at least the total of alac_hip_resample_frames
 *   out_channel_stride  floats from one row to the next, at least out_frames
 *   d_reports         [num_segments] alac_hip_resample_report, 8-byte aligned; every word is written by every call
 * Asynchronous on the context's stream.  kALAC_ParamError, with nothing enqueued and nothing written: everything the loudness
 * call refuses in the source, num_channels and the table; a bad rate pair; a null or misaligned workspace, or one that is too
 * small; a null or misaligned d_out or d_reports; out_frames below the total; out_channel_stride below out_frames.
 */
typedef struct alac_hip_resample_report { /* one per segment, 32 bytes */
    uint64_t out_first;  /* the segment's first output frame in a row of d_out */
    uint64_t out_frames; /* its output frames: ceil(N * L / M) */
    double peak;         /* the largest |float32 written| of the segment, exact; above 1.0: alac_hip_encode_float will clip */
    uint64_t nonfinite;  /* non-finite input samples of the segment, read as 0.0 */
} alac_hip_resample_report;
/* Host only, no context: L, M and K of a rate pair, and with out_coefs not null the coefficients h_p[k] in out_coefs [L * K],
 * phase-major (out_coefs null: the sizes alone).  The kernels take their coefficients from here.  kALAC_ParamError for a bad
 * pair or a null out_L, out_M or out_K. */
int32_t alac_hip_resample_filter(uint32_t in_rate, uint32_t out_rate, uint32_t *out_L, uint32_t *out_M, uint32_t *out_K,
                                 double *out_coefs);
/* Host only, no context: the output frames of all segments back to back; h_out_first [num_segments + 1] (may be null) gets
 * every segment's first output frame and the total.  h_seg_first_frame null: one segment of total_frames.  Returns 0 and
 * writes nothing for a bad rate pair, num_segments 0 or a table the calls refuse. */
uint64_t alac_hip_resample_frames(uint32_t in_rate, uint32_t out_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                  uint32_t num_segments, uint64_t *h_out_first);
uint64_t alac_hip_resample_workspace_bytes(uint32_t in_rate, uint32_t out_rate, uint32_t num_channels, uint32_t num_segments);
int32_t alac_hip_resample_int(alac_hip_ctx *ctx, const void *d_in, const alac_hip_int_source *src, uint32_t num_channels,
                              uint32_t in_rate, uint32_t out_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                              uint32_t num_segments, void *d_workspace, uint64_t workspace_bytes, float *d_out,
                              uint64_t out_channel_stride, uint64_t out_frames, alac_hip_resample_report *d_reports);
int32_t alac_hip_resample_float(alac_hip_ctx *ctx, const float *d_in, uint32_t num_channels, uint64_t channel_stride,
                                uint64_t frame_stride, uint32_t in_rate, uint32_t out_rate, uint64_t total_frames,
                                const uint64_t *h_seg_first_frame, uint32_t num_segments, void *d_workspace,
                                uint64_t workspace_bytes, float *d_out, uint64_t out_channel_stride, uint64_t out_frames,
                                alac_hip_resample_report *d_reports);
/* Host-buffer forms (synchronous): h_in in the layout above, staged as the loudness host forms stage it; the rows come back in
 * h_out (channel c's frame j at h_out[c * out_channel_stride + j]), the reports in h_reports [num_segments]. */
int32_t alac_hip_resample_int_host(alac_hip_ctx *ctx, const void *h_in, const alac_hip_int_source *src, uint32_t num_channels,
                                   uint32_t in_rate, uint32_t out_rate, uint64_t total_frames, const uint64_t *h_seg_first_frame,
                                   uint32_t num_segments, float *h_out, uint64_t out_channel_stride, uint64_t out_frames,
                                   alac_hip_resample_report *h_reports);
int32_t alac_hip_resample_float_host(alac_hip_ctx *ctx, const float *h_in, uint32_t num_channels, uint64_t channel_stride,
                                     uint64_t frame_stride, uint32_t in_rate, uint32_t out_rate, uint64_t total_frames,
                                     const uint64_t *h_seg_first_frame, uint32_t num_segments, float *h_out,
                                     uint64_t out_channel_stride, uint64_t out_frames, alac_hip_resample_report *h_reports);

/* Parse a magic cookie into a format (host only). */
int32_t alac_hip_format_from_cookie(const uint8_t *h_cookie, uint32_t cookie_size,
                                    alac_hip_format *out_fmt);

/* ---- stage-level entry points (device buffers), the extern "C" surface of
 *      codec/dplib.h:49-55, codec/aglib.h:70-74, codec/matrixlib.h:41-60, batched -------------- */

/* pc_block over num_rows independent rows: row r reads d_in + r*row_stride (int32), writes
 * d_pc + r*row_stride (positions < num), adapts d_coefs + r*32 (int16, numactive used) in place
 * (codec/dp_enc.c:77).  row_stride must cover max(num, numactive + 1) readable samples. */
int32_t alac_hip_pc_block(alac_hip_ctx *ctx, const int32_t *d_in, int32_t *d_pc, uint32_t num_rows,
                          uint32_t row_stride, int32_t num, int16_t *d_coefs, int32_t numactive,
                          uint32_t chanbits, uint32_t denshift);
/* unpc_block, same layout (codec/dp_dec.c:55). */
int32_t alac_hip_unpc_block(alac_hip_ctx *ctx, const int32_t *d_pc, int32_t *d_out,
                            uint32_t num_rows, uint32_t row_stride, int32_t num, int16_t *d_coefs,
                            int32_t numactive, uint32_t chanbits, uint32_t denshift);
/* dyn_comp over num_rows rows with AG params (mb0, pb, kb): row r codes num_samples residuals of
 * d_pc + r*row_stride into d_bits + r*bytes_stride starting at bit 0; bit counts to d_num_bits
 * (codec/ag_enc.c:249).  d_bits may be NULL to count only. */
int32_t alac_hip_dyn_comp(alac_hip_ctx *ctx, uint32_t mb0, uint32_t pb, uint32_t kb,
                          const int32_t *d_pc, uint32_t num_rows, uint32_t row_stride,
                          int32_t num_samples, int32_t bit_size, uint8_t *d_bits,
                          uint32_t bytes_stride, uint32_t *d_num_bits);
/* dyn_decomp, inverse layout (codec/ag_dec.c:272); per-row status to d_status. */
int32_t alac_hip_dyn_decomp(alac_hip_ctx *ctx, uint32_t mb0, uint32_t pb, uint32_t kb,
                            const uint8_t *d_bits, uint32_t bytes_stride, uint32_t num_rows,
                            int32_t *d_pc, uint32_t row_stride, int32_t num_samples,
                            int32_t max_size, uint32_t *d_num_bits, int32_t *d_status);

/* ---- host-buffer convenience (synchronous; does its own H2D/D2H and scratch) -----------------
 * What ALACEncoder::Encode / ALACDecoder::Decode callers with host buffers use
 * (convert-utility/main.cu:558, :719). */
int32_t alac_hip_encode_host(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *h_pcm,
                             uint64_t total_samples, uint32_t segment_packets, int16_t *h_state,
                             int32_t state_in, uint8_t *h_out, uint64_t out_capacity,
                             uint32_t *h_packet_bytes, uint64_t *out_total_bytes);
/* General form: packets back to back at the full-packet stride, packet p holding h_num_samples[p] frames;
 * segment s = packets [h_seg_first[s], h_seg_first[s+1]) chained through the coefficient state (one
 * segment per input file in a multi-file conversion).  h_state: num_segments * 64 int16, may be NULL. */
int32_t alac_hip_encode_host_segments(alac_hip_ctx *ctx, const alac_hip_format *fmt, const void *h_pcm,
                                      const uint32_t *h_num_samples, uint32_t num_packets,
                                      const uint32_t *h_seg_first, uint32_t num_segments, int16_t *h_state,
                                      int32_t state_in, uint8_t *h_out, uint64_t out_capacity,
                                      uint32_t *h_packet_bytes, uint64_t *out_total_bytes);
int32_t alac_hip_decode_host(alac_hip_ctx *ctx, const uint8_t *h_cookie, uint32_t cookie_size,
                             const uint8_t *h_stream, const uint32_t *h_packet_bytes,
                             uint32_t num_packets, uint8_t *h_pcm_out, uint32_t *h_num_samples_out,
                             int32_t *h_status);

/* ---- deterministic synthetic PCM, host side --------------------------------- */
void alac_synth_frame(uint64_t frame_index, uint32_t num_samples, uint32_t bit_depth,
                      uint32_t channels, uint8_t *h_out);
void alac_synth_pcm(uint64_t first_frame, uint32_t num_frames, uint32_t frame_size,
                    uint32_t bit_depth, uint32_t channels, uint8_t *h_out);
/* The same generator on the device (same source, same bytes): frames [first_frame, first_frame + num_frames) of
 * fmt->frame_size sample-frames each, written back to back at d_out on the context's stream (1 or 2 channels).
 * BASELINE.json configs[3]: every rank generates its own shard in HBM. */
int32_t alac_hip_synth_pcm(alac_hip_ctx *ctx, uint64_t first_frame, uint32_t num_frames,
                           const alac_hip_format *fmt, uint8_t *d_out);

/* ---- sharding across GPUs, host only ------------------------------------------------------
 * One process per GPU encodes a contiguous range of the independent units (segments / packets); the shards are byte
 * aligned (codec/ALACEncoder.cu:1039), so the stream is their concatenation in rank order.
 * alac_hip_shard_range: rank `rank` of `world` takes units [*first, *first + *count); the ranges tile [0, num_units).
 * alac_hip_shard_offsets: offsets[r] = byte position of rank r's shard in the re-assembled stream, offsets[world] = its
 * length (the exclusive prefix sum of the all-gathered shard sizes).  Both return 0 or kALAC_ParamError. */
int32_t alac_hip_shard_range(uint64_t num_units, uint32_t world, uint32_t rank, uint64_t *first, uint64_t *count);
int32_t alac_hip_shard_offsets(const uint64_t *shard_bytes, uint32_t world, uint64_t *offsets);

/* ---- stream re-assembly across the GPUs of one node, on RCCL (alac_comm.cpp) ------------------
 * BASELINE north_star: "frames are sharded across the 8 GPUs of one node with RCCL all-gather over xGMI to reassemble the
 * stream".  No reference counterpart (the fork is single-GPU); what makes it legal is the byte alignment of every packet
 * (codec/ALACEncoder.cu:1039).  One process per GPU, one alac_hip_comm per process; librccl is loaded on first use.
 *   alac_hip_comm_unique_id   rank 0 makes the 128-byte ncclUniqueId and hands it to the other ranks by whatever channel
 *                             the launcher has (a file, a socket, torch.distributed's store)
 *   alac_hip_comm_create      ncclCommInitRank on `device`; collective over all `world` ranks.  kALAC_UnimplementedError
 *                             if librccl cannot be loaded
 * Re-assembly of one pass, two phases so that a pipelined caller never waits for the GPU between two encodes; `slot`
 * (0 .. ALAC_HIP_COMM_SLOTS-1) names the pass while both are outstanding:
 *   alac_hip_reassemble_begin   enqueues on `stream` (hipStream_t): all-gather of {shard bytes, shard capacity, output
 *                             capacity} and — when d_packet_bytes is given — of the per-packet sizes into d_all_packet_bytes
 *                             [world * num_packets] (equal num_packets on every rank: the CAF 'pakt' table of the whole
 *                             stream); the table's copy to pinned host memory and an event.  d_shard_bytes: device pointer
 *                             to this rank's byte count (d_packet_offsets + num_packets of alac_hip_encode).  No host wait.
 *   alac_hip_reassemble_finish  waits for that event only, computes the offsets (alac_hip_shard_offsets; copied to
 *                             h_offsets[world + 1] when non-NULL), and enqueues ONE group on `stream`: ncclRecv of every
 *                             peer's shard straight at its offset in d_stream_out, ncclSend of d_shard to every peer, the
 *                             own shard as a device copy.  kALAC_ParamError — on EVERY rank alike, before anything is
 *                             posted — if a shard is longer than its buffer or the stream longer than any rank's
 *                             out_capacity.
 *   alac_hip_reassemble       both phases back to back (slot 0). */
typedef struct alac_hip_comm alac_hip_comm;
#define ALAC_HIP_COMM_ID_BYTES 128
#define ALAC_HIP_COMM_SLOTS 4
int32_t alac_hip_comm_unique_id(uint8_t *h_id);
int32_t alac_hip_comm_create(alac_hip_comm **out_comm, int32_t device, const uint8_t *h_id, uint32_t rank, uint32_t world);
void alac_hip_comm_destroy(alac_hip_comm *comm);
uint32_t alac_hip_comm_rank(const alac_hip_comm *comm);
uint32_t alac_hip_comm_world(const alac_hip_comm *comm);
const char *alac_hip_comm_last_error(const alac_hip_comm *comm);
int32_t alac_hip_reassemble_begin(alac_hip_comm *comm, uint32_t slot, const uint64_t *d_shard_bytes, uint64_t shard_capacity,
                                  uint64_t out_capacity, const uint32_t *d_packet_bytes, uint32_t num_packets,
                                  uint32_t *d_all_packet_bytes, void *stream);
int32_t alac_hip_reassemble_finish(alac_hip_comm *comm, uint32_t slot, const uint8_t *d_shard, uint8_t *d_stream_out,
                                   uint64_t *h_offsets, void *stream);
int32_t alac_hip_reassemble(alac_hip_comm *comm, const uint8_t *d_shard, const uint64_t *d_shard_bytes, uint64_t shard_capacity,
                            const uint32_t *d_packet_bytes, uint32_t num_packets, uint32_t *d_all_packet_bytes,
                            uint8_t *d_stream_out, uint64_t out_capacity, uint64_t *h_offsets, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ALAC_HIP_H */
