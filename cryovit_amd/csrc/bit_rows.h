// A bit per voxel of a [D][H][W] volume, one uint64 per 64 voxels of a row: [D][H][WW] words, WW = words_per_row(W), bit i of word w
// of a row = voxel x = 64 w + i; bits past W are 0 in what a pack kernel writes.  Shared by cleanup.hip (the flood), curvature.hip
// and picks.hip: the extents with the word count, the bytes of one bitmap (what both *_workspace_bytes entries return), the word
// and voxel a wave of a pack kernel owns, the mask of a row's last word, the discrete ball as half-widths along x, a span of a row
// of words as one word, and the slot of a bit in the raster-order LDS queue of the 4x8x64-tile kernels.  Every includer compiles its own copy.
#pragma once
#include "entry_checks.h"

namespace cvx {

typedef unsigned long long Word;

__host__ __device__ constexpr int words_per_row(int W) { return W / 64 + (W % 64 != 0); }

// of the kernels that walk the volume in the 4x8x64 tiles of voxel_rows.h: a tile is one word of 32 rows
struct BitDims {
    int D, H, W, WW;
    int tx, ty;  // tiles along x and y
};

inline BitDims bit_dims(int D, int H, int W) {
    const Dims d = ccl_dims(D, H, W);
    return BitDims{D, H, W, words_per_row(W), d.tx, d.ty};
}

inline long bitmap_words(const BitDims& d) { return (long)d.D * d.H * d.WW; }
inline long bitmap_bytes(const BitDims& d) { return bitmap_words(d) * (long)sizeof(Word); }

// what cvx_curvature_workspace_bytes and cvx_pick_workspace_bytes return: the bytes of one bitmap, -1 for extents they refuse
inline long bitmap_workspace_bytes(int D, int H, int W) {
    long n = 0;
    if (extents_fault(D, H, W, kExtentMax, n)) return -1;
    return bitmap_bytes(bit_dims(D, H, W));
}

// a pack kernel runs one wave per word: the blocks of `waves` waves
inline unsigned wave_blocks_of(long waves) { return (unsigned)((waves + kCclThreads / 64 - 1) / (kCclThreads / 64)); }

// g = the word of this wave, row = z * H + y of its row, x = the voxel of this lane (at or past W in a ragged last word: the
// caller tests it before it reads).  false past the bitmap, for the whole wave alike
__device__ __forceinline__ bool wave_word(int WW, long words, long& g, long& row, int& x) {
    const int lane = threadIdx.x & 63;
    g = (long)blockIdx.x * (kCclThreads / 64) + (threadIdx.x >> 6);
    if (g >= words) return false;
    row = g / WW;
    x = (int)(g % WW) * 64 + lane;
    return true;
}

// the bits of a row's last word that are voxels
__host__ __device__ __forceinline__ Word tail_mask(int W) { return W % 64 ? (1ull << W % 64) - 1 : ~0ull; }

// the half-width along x of the ball {o : |o|^2 <= R2} in the row (az, ay); -1: the row is outside
__host__ __device__ __forceinline__ int ball_half_width(int R2, int az, int ay) {
    const int rem = R2 - az * az - ay * ay;
    if (rem < 0) return -1;
    int w = 0;
    while ((w + 1) * (w + 1) <= rem) ++w;
    return w;
}

// the bits lo .. lo + 2w of a row of `words` words, as bits 0 .. 2w; 0 <= lo, lo + 2w < 64 * words, w <= 16
__device__ __forceinline__ Word row_span(const Word* p, int words, int lo, int w) {
    const int i0 = lo >> 6, sh = lo & 63;
    Word v = p[i0] >> sh;
    if (sh && i0 + 1 < words) v |= p[i0 + 1] << (64 - sh);
    return v & ((2ull << (2 * w)) - 1);
}

// The LDS queue of a tile kernel holds the set bits of its rows' words in raster order, without atomics: thread 0 writes first[f] =
// the entries before row f (a prefix sum over the rows' popcounts), then bit `lane` of a row's word m whose first entry is at
// `first` has the slot
__device__ __forceinline__ int queue_slot(int first, Word m, int lane) { return first + __popcll(m & ((1ull << lane) - 1)); }

}  // namespace cvx
