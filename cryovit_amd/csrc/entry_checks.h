// What the entry points of the analysis passes (components, edt, nearest, overlap, split, shape, skeleton, thickness, mesh, cleanup,
// curvature, picks) check and compute on the host before they launch: the extents of the volume, the clamp of an id count, the
// block and tile counts of a launch, whether k table rows can be addressed.  Refusals go through cvx_fail(entry, why) of
// host_util.h.  cleanup, curvature and picks include it through bit_rows.h, which adds the word and byte counts of a bitmap.
#pragma once
#include "voxel_rows.h"
#include "host_util.h"

#include <limits.h>

namespace cvx {

constexpr int kExtentMax = 32768;  // of the passes that hold a coordinate in 15 bits; extents_fault's text names it
constexpr int kExtentAny = INT_MAX;
// the one sentence the entries without that cap give for every fault of the extents
constexpr const char* kExtentsRule = "extents must be >= 0 with D*H*W <= 2^31 - 2";

// what is wrong with the extents, or nullptr: none negative, none above cap, D*H*W <= CVX_COMPONENT_MAX_VOXELS.  n = D*H*W
inline const char* extents_fault(int D, int H, int W, int cap, long& n) {
    if (D < 0 || H < 0 || W < 0) return "negative extent";
    if (D > cap || H > cap || W > cap) return "an extent above 32768";
    n = (long)D * H;  // < 2^62
    if (W && n > CVX_COMPONENT_MAX_VOXELS / W) return "D*H*W must be <= 2^31 - 2";
    n *= W;
    return nullptr;
}

inline int clamp_int(long k) { return (int)(k < INT_MAX ? k : INT_MAX); }  // ids: an int32 label is never above it
inline unsigned blocks_of(long items) { return (unsigned)((items + kCclThreads - 1) / kCclThreads); }
inline long tile_count(const Dims& d) { return (long)d.tx * d.ty * ((d.D + TZ - 1) / TZ); }  // <= D*H*W
inline bool rows_fit(long k, int cols) { return k <= LONG_MAX / (cols * (long)sizeof(int64_t)); }

}  // namespace cvx
