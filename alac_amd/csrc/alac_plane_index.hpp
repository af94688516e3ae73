// alac_plane_index.hpp — the one layout of the encoder's residual planes (resA / resB / resC, alac_encode_v1_types.hpp):
// [sample / 4][stream][4].  Four consecutive residuals of a stream are 16 aligned bytes (one cell), consecutive streams are
// consecutive cells, and a "group row" (the cells of every stream for four samples) is stride * 16 bytes.  The predictor
// waves hand a chain's residuals over in 16-byte stores and the coder lanes fetch them in 16-byte loads; every writer and
// reader of the planes, in every regime, indexes through plane_index.
// A host compiler sees this file alone (tests/cpp/plane_index.cpp).
#pragma once

#include <stdint.h>
#if defined(__HIPCC__)
#define ALAC_PLANE_FN __host__ __device__ __forceinline__
#else
#define ALAC_PLANE_FN inline
#endif

namespace alacdev {

constexpr uint32_t kPlaneGroup = 4;  // samples per cell

// int32 index of (sample j, stream s) in a plane of `stride` streams
ALAC_PLANE_FN uint64_t plane_index(uint64_t j, uint64_t stride, uint64_t s)
{
    return ((j >> 2) * stride + s) * kPlaneGroup + (j & 3);
}

// the plane seen from stream `first` on: stream s of the result is stream first + s of `plane`, same stride
template <class T>
ALAC_PLANE_FN T *plane_from_stream(T *plane, uint64_t first)
{
    return plane + first * kPlaneGroup;
}

// rows a plane of `rows` samples occupies (whole groups)
ALAC_PLANE_FN uint64_t plane_rows(uint64_t rows) { return (rows + kPlaneGroup - 1) & ~(uint64_t)(kPlaneGroup - 1); }

}  // namespace alacdev
