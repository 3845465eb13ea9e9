// Cleaning a predicted uint8 mask before it is labelled (`--close-radius`, `--fill-holes`, `--open-radius`): the border flood
// behind "fill holes", the threshold of a distance map behind dilation and erosion by a Euclidean ball (edt.hip makes the map,
// the layer above chains the steps), and the per-instance count of the voxels the cleaning added.  Integers only; no result
// depends on scheduling.
//
// FILL.  A background voxel stays background iff it is connected to the border through background.  The flood runs on bits: one
// uint64 per 64 voxels of a row (bit i of word w = voxel x = 64 w + i; WW = ceil(W / 64) words per row), `open` = the mask is 0,
// `reach` = open and connected to the border as far as known.  128x512x512 is 4 MB of either.
//   k_mask_pack    a wave reads 64 bytes of a row, one __ballot is the open word; reach starts as the open bits of the border (the
//                  six faces, or with `slices` the four edges of every z-slice).  Bits past W are never open.
//   k_mask_round   a workgroup owns 4 x 16 rows x 8 words, loads reach with a halo of one row and one word into LDS and repeats
//                      reach' = open & fill_x(reach | rows above / below / before / behind [| those rows shifted by one bit])
//                  until its tile stops changing or kFloodSweeps sweeps are done.  fill_x spreads the set bits along the open runs
//                  of the word in six shift-and-mask steps each way (Kogge-Stone occluded fill); a run that goes on in the next
//                  word gets there by that word's edge bit.  With background connectivity 26 the eight rows around are also
//                  taken shifted by +-1 bit, with the edge bit of the word beside; `slices` drops the rows of other planes.  The
//                  workgroup stores the words of its own tile that grew (one aligned 8-B store each) and raises the round's flag.
//                  Bits are only ever set and every set bit is reachable, so a halo read early or late is a subset of the
//                  truth: the order decides how many rounds it takes, never the result.  It waits for no other workgroup.  The
//                  host launches rounds until one raises no flag: every tile was then stable against halos nobody changed,
//                  which is the fixpoint, and the fixpoint is the reachable set.
//   k_mask_unpack  out = 1 - reach as bytes, 16 voxels per thread (a voxel that is not reached is foreground or a filled hole).
// BALL STEPS.  k_mask_threshold turns an int32 distance map into the uint8 mask d2 <= t (dilation, from the map to the nonzero
// voxels) or d2 > t (erosion, from the map to the zero voxels; CVX_EDT_NONE, "no zero voxel anywhere", is above every t), and
// crops `pad` voxels from every side of the map on the way: the closing runs on a zero-padded copy.
// ADDED VOXELS.  k_mask_added walks labels and the mask as predicted in 4x8x64 tiles and counts per id the voxels that mask did
// not have, with the per-id reduction of voxel_rows.h.
#include "bit_rows.h"

namespace cvx {

constexpr int FZ = 4, FY = 16, FW = 8;             // the flood tile: planes, rows, words of a row
constexpr int GZ = FZ + 2, GY = FY + 2, GW = FW + 2;  // with its halo
constexpr int kFloodCells = GZ * GY * GW;          // 1080 words = 8.4 KB
constexpr int kFloodOwn = FZ * FY * FW / kCclThreads;  // own words per thread
constexpr int kFloodSweeps = 16;                   // per round: a straight crossing of the tile; a winding one goes on in the next round
static_assert(FZ * FY * FW % kCclThreads == 0, "every thread owns the same number of words");

struct FloodDims {
    int D, H, W, WW;
    int tw, ty;  // tiles along x (in words) and y
};

inline FloodDims flood_dims(int D, int H, int W) {
    const int WW = words_per_row(W);
    return FloodDims{D, H, W, WW, (WW + FW - 1) / FW, (H + FY - 1) / FY};
}
inline long flood_tiles(const FloodDims& d) { return (long)d.tw * d.ty * ((d.D + FZ - 1) / FZ); }  // <= D*H*WW <= D*H*W

__device__ __forceinline__ Word ld_word_lds(const Word* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void st_word_lds(Word* p, Word v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ Word ld_word_dev(const Word* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_word_dev(Word* p, Word v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one wave per word
__global__ __launch_bounds__(kCclThreads) void k_mask_pack(const uint8_t* __restrict__ mask, FloodDims d, long words, int slices,
                                                           Word* __restrict__ open, Word* __restrict__ reach) {
    long g, row;
    int x;
    if (!wave_word(d.WW, words, g, row, x)) return;
    const Word o = __ballot(x < d.W && mask[row * d.W + x] == 0);
    if ((threadIdx.x & 63) != 0) return;
    const int w = (int)(g % d.WW), y =(int)(row % d.H), z = (int)(row / d.H);
    Word seed = 0;  // the border voxels of this word
    if (y == 0 || y == d.H - 1 || (!slices && (z == 0 || z == d.D - 1))) seed = ~0ull;
    if (w == 0) seed |= 1ull;
    if (w == d.WW - 1) seed |= 1ull << ((d.W - 1) & 63);
    open[g] = o;
    reach[g] = o & seed;
}

// the bits of `pro` that a walk from a bit of `gen` reaches over set bits of `pro`, towards higher and towards lower bits
__device__ __forceinline__ Word fill_x(Word gen, Word pro) {
    Word up = gen & pro, dn = up, pu = pro, pd = pro;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        up |= pu & (up << s);
        pu &= pu << s;
        dn |= pd & (dn >> s);
        pd &= pd >> s;
    }
    return up | dn;
}

template <int BACKGROUND, bool SLICES>
__global__ __launch_bounds__(kCclThreads) void k_mask_round(const Word* __restrict__ open, Word* __restrict__ reach, FloodDims d,
                                                            int* __restrict__ changed) {
    __shared__ Word cell[kFloodCells];
    const int b = blockIdx.x;
    const int w0 = (b % d.tw) * FW, y0 = (b / d.tw % d.ty) * FY, z0 = (b / d.tw / d.ty) * FZ;
    // the own words: open, and whether one is left to reach at all
    Word own_open[kFloodOwn];
    int at[kFloodOwn];  // the LDS cell of the own word
    int todo = 0;
#pragma unroll
    for (int k = 0; k < kFloodOwn; ++k) {
        const int li = threadIdx.x + k * kCclThreads;
        const int lw = li % FW, ly = li / FW % FY, lz = li / (FW * FY);
        at[k] = ((lz + 1) * GY + ly + 1) * GW + lw + 1;
        const int w = w0 + lw, y = y0 + ly, z = z0 + lz;
        const bool in = w < d.WW && y < d.H && z < d.D;
        const long g = ((long)z * d.H + y) * d.WW + w;
        own_open[k] = in ? open[g] : 0;
        todo |= in && (own_open[k] & ~ld_word_dev(reach + g)) != 0;
    }
    if (!__syncthreads_or(todo)) return;  // every open voxel of the tile is reached already (or there is none)
    // reach with the halo; a cell outside the volume reaches nothing
    for (int c = threadIdx.x; c < kFloodCells; c += kCclThreads) {
        const int w = w0 - 1 + c % GW, y = y0 - 1 + c / GW % GY, z = z0 - 1 + c / (GW * GY);
        const bool in = (unsigned)w < (unsigned)d.WW && (unsigned)y < (unsigned)d.H && (unsigned)z < (unsigned)d.D;
        cell[c] = in ? ld_word_dev(reach + ((long)z * d.H + y) * d.WW + w) : 0;
    }
    __syncthreads();
    // sweeps inside LDS.  Other waves set bits meanwhile; whatever a read returns is a set of reachable voxels.
    unsigned grew = 0;  // bit k: own word k ends above the value it was loaded with
    for (int sweep = 0; sweep < kFloodSweeps; ++sweep) {
        int moved = 0;
#pragma unroll
        for (int k = 0; k < kFloodOwn; ++k) {
            const Word o = own_open[k];
            if (o == 0) continue;
            const Word* p = cell + at[k];
            const Word mine = ld_word_lds(p);
            if (mine == o) continue;
            // the rows around, and the words before and behind them
            Word u = 0, ul = 0, ur = 0;
#pragma unroll
            for (int dz = SLICES ? 0 : -1; dz <= (SLICES ? 0 : 1); ++dz)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy) {
                    if (dz == 0 && dy == 0) continue;
                    if (BACKGROUND == 6 && dz != 0 && dy != 0) continue;
                    const Word* q = p + (dz * GY + dy) * GW;
                    u |= ld_word_lds(q);
                    if (BACKGROUND == 26) {
                        ul |= ld_word_lds(q - 1);
                        ur |= ld_word_lds(q + 1);
                    }
                }
            Word gen = mine | u | ld_word_lds(p - 1) >> 63 | ld_word_lds(p + 1) << 63;
            if (BACKGROUND == 26) gen |= u << 1 | ul >> 63 | u >> 1 | ur << 63;
            const Word next = fill_x(gen, o);  // holds mine: mine is a subset of o
            if (next != mine) {
                st_word_lds(cell + at[k], next);
                grew |= 1u << k;
                moved = 1;
            }
        }
        if (!__syncthreads_or(moved)) break;
    }
    // only this workgroup writes its own words
#pragma unroll
    for (int k = 0; k < kFloodOwn; ++k) {
        if (!(grew >> k & 1)) continue;
        const int li = threadIdx.x + k * kCclThreads;
        const int lw = li % FW, ly = li / FW % FY, lz = li / (FW * FY);
        st_word_dev(reach + ((long)(z0 + lz) * d.H + y0 + ly) * d.WW + w0 + lw, cell[at[k]]);  // grew => open => inside the volume
    }
    if (__syncthreads_or(grew != 0) && threadIdx.x == 0) *changed = 1;
}

// v[0..cnt) as bytes to p: one 16-B store for a full, 16-B aligned group.  bits: bit i = v[i]
__device__ __forceinline__ void bytes_store(uint8_t* __restrict__ p, int cnt, unsigned bits) {
    if (cnt == RV && ((uintptr_t)p & 15) == 0) {
        unsigned q[RV / 4];
#pragma unroll
        for (int j = 0; j < RV / 4; ++j) {
            const unsigned nib = bits >> (4 * j) & 15u;
            q[j] = (nib & 1u) | (nib & 2u) << 7 | (nib & 4u) << 14 | (nib & 8u) << 21;
        }
        *(uint4*)p = uint4{q[0], q[1], q[2], q[3]};
    } else {
#pragma unroll
        for (int i = 0; i < RV; ++i)
            if (i < cnt) p[i] = bits >> i & 1u;
    }
}

__global__ __launch_bounds__(kCclThreads) void k_mask_unpack(const Word* __restrict__ reach, Dims d, int WW, int segs, uint8_t* __restrict__ out) {
    static_assert(64 % RV == 0, "a row piece lies in one word");
    long row;
    int x0, cnt;
    if (!row_piece(d, segs, row, x0, cnt)) return;
    const unsigned bits = (unsigned)(~reach[row * WW + x0 / 64] >> (x0 & 63)) & 0xffffu;
    bytes_store(out + row * d.W + x0, cnt, bits);
}

// d: the extents of out; the map has `pad` voxels more on every side
template <int MODE>
__global__ __launch_bounds__(kCclThreads) void k_mask_threshold(const int* __restrict__ d2, Dims d, int pad, int thr, int segs,
                                                                uint8_t* __restrict__ out) {
    int z, y, x0, cnt;
    if (!row_piece(d, segs, z, y, x0, cnt)) return;
    const long ph = d.H + 2 * (long)pad, pw = d.W + 2 * (long)pad;
    int v[RV];
    row_load(d2 + ((z + pad) * ph + y + pad) * pw + pad + x0, cnt, v);
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < RV; ++i) bits |= (unsigned)(MODE == CVX_MASK_LE ? v[i] <= thr : v[i] > thr) << i;  // thr < CVX_EDT_NONE
    bytes_store(out + ((long)z * d.H + y) * d.W + x0, cnt, bits);
}

__global__ __launch_bounds__(kCclThreads) void k_mask_added(const int* __restrict__ labels, const uint8_t* __restrict__ before,
                                                            long long* __restrict__ out, Dims d, int k) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    int z0, y0, x0;
    tile_origin(d, z0, y0, x0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = z0 + wave, x = x0 + lane;
    long long acc[1] = {0};
    int cur = 0;  // the id acc belongs to; 0: none yet
    if (z < d.D && x < d.W)
        for (int yy = 0; yy < TY && y0 + yy < d.H; ++yy) {
            const long v = ((long)z * d.H + y0 + yy) * d.W + x;
            const int id = labels[v];
            if (id < 1 || id > k || before[v] != 0) continue;
            if (id != cur) {
                if (cur) table_flush(out, cur, acc);
                cur = id;
            }
            acc[0] += 1;
        }
    // the wave: one id among the threads that hold one?  Then lane 0 sends the wave's sum; else every thread sends its own
    const int one = wave_single_id(cur);
    if (!one) {
        if (cur) table_flush(out, cur, acc);
        return;
    }
    acc[0] = wave_sum(acc[0]);
    if (lane == 0) table_flush(out, one, acc);
}

}  // namespace cvx

using namespace cvx;

namespace {

// what the flood entries refuse about the volume and their two word arrays; nullptr: fine
const char* flood_fault(int D, int H, int W, const void* open, const void* reach, long& n) {
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return why;
    if (n > 0 && (!open || !reach)) return "null pointer";
    if (((uintptr_t)open | (uintptr_t)reach) & 7) return "open and reach must be 8-B aligned";
    return nullptr;
}

}  // namespace

extern "C" int cvx_mask_flood_pack(const uint8_t* mask, int D, int H, int W, int slices, uint64_t* open, uint64_t* reach, hipStream_t st) {
    long n = 0;
    if (const char* why = flood_fault(D, H, W, open, reach, n)) return cvx_fail("mask_flood_pack", why);
    if (slices != 0 && slices != 1) return cvx_fail("mask_flood_pack", "slices must be 0 or 1");
    if (n == 0) return 0;
    if (!mask) return cvx_fail("mask_flood_pack", "null pointer");
    if (open == reach) return cvx_fail("mask_flood_pack", "open and reach must be different arrays");
    const FloodDims d = flood_dims(D, H, W);
    const long words = (long)D * H * d.WW;
    hipLaunchKernelGGL(k_mask_pack, dim3(wave_blocks_of(words)), dim3(kCclThreads), 0, st, mask, d, words, slices, (Word*)open, (Word*)reach);
    return cvx_check_launch();
}

extern "C" int cvx_mask_flood_rounds(const uint64_t* open, uint64_t* reach, int D, int H, int W, int background, int slices, int rounds,
                                     int32_t* changed, hipStream_t st) {
    long n = 0;
    if (const char* why = flood_fault(D, H, W, open, reach, n)) return cvx_fail("mask_flood_rounds", why);
    if (background != 6 && background != 26) return cvx_fail("mask_flood_rounds", "background must be 6 or 26");
    if (slices != 0 && slices != 1) return cvx_fail("mask_flood_rounds", "slices must be 0 or 1");
    if (rounds < 1) return cvx_fail("mask_flood_rounds", "rounds < 1");
    if (!changed) return cvx_fail("mask_flood_rounds", "null pointer");
    if ((uintptr_t)changed & 3) return cvx_fail("mask_flood_rounds", "changed must be 4-B aligned");
    if (n == 0) return 0;  // nothing to flood and nothing launched: the caller does not read changed
    if (open == reach) return cvx_fail("mask_flood_rounds", "open and reach must be different arrays");
    CVX_HIP(hipMemsetAsync(changed, 0, (size_t)rounds * sizeof(int), st));
    const FloodDims d = flood_dims(D, H, W);
    const dim3 grid((unsigned)flood_tiles(d)), block(kCclThreads);
    for (int r = 0; r < rounds; ++r) {
        const Word* o = (const Word*)open;
        Word* q = (Word*)reach;
        if (background == 26 && slices) hipLaunchKernelGGL((k_mask_round<26, true>), grid, block, 0, st, o, q, d, changed + r);
        else if (background == 26) hipLaunchKernelGGL((k_mask_round<26, false>), grid, block, 0, st, o, q, d, changed + r);
        else if (slices) hipLaunchKernelGGL((k_mask_round<6, true>), grid, block, 0, st, o, q, d, changed + r);
        else hipLaunchKernelGGL((k_mask_round<6, false>), grid, block, 0, st, o, q, d, changed + r);
        if (const int rc = cvx_check_launch()) return rc;
    }
    return 0;
}

extern "C" int cvx_mask_flood_unpack(const uint64_t* reach, int D, int H, int W, uint8_t* out, hipStream_t st) {
    long n = 0;
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("mask_flood_unpack", why);
    if (n == 0) return 0;
    if (!reach || !out) return cvx_fail("mask_flood_unpack", "null pointer");
    if ((uintptr_t)reach & 7) return cvx_fail("mask_flood_unpack", "reach must be 8-B aligned");
    const int segs = (W + RV - 1) / RV;
    hipLaunchKernelGGL(k_mask_unpack, dim3(blocks_of((long)D * H * segs)), dim3(kCclThreads), 0, st, (const Word*)reach, ccl_dims(D, H, W),
                       flood_dims(D, H, W).WW, segs, out);
    return cvx_check_launch();
}

extern "C" int cvx_mask_threshold(const int32_t* d2, int D, int H, int W, int pad, int mode, int threshold_d2, uint8_t* out, hipStream_t st) {
    long n = 0, padded = 0;
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("mask_threshold", why);
    if (pad < 0 || pad > kExtentMax) return cvx_fail("mask_threshold", "pad must lie in [0, 32768]");
    const long pd = D + 2L * pad, ph = H + 2L * pad, pw = W + 2L * pad;
    if (pd > INT_MAX || ph > INT_MAX || pw > INT_MAX || extents_fault((int)pd, (int)ph, (int)pw, kExtentAny, padded))
        return cvx_fail("mask_threshold", "the padded extents must have (D+2*pad)*(H+2*pad)*(W+2*pad) <= 2^31 - 2");
    if (mode != CVX_MASK_LE && mode != CVX_MASK_GT) return cvx_fail("mask_threshold", "mode must be CVX_MASK_LE or CVX_MASK_GT");
    if (threshold_d2 < 0 || threshold_d2 == CVX_EDT_NONE) return cvx_fail("mask_threshold", "threshold_d2 must lie in [0, 2^31 - 2]");
    if (n == 0) return 0;
    if (!d2 || !out) return cvx_fail("mask_threshold", "null pointer");
    if ((uintptr_t)d2 & 3) return cvx_fail("mask_threshold", "d2 must be 4-B aligned");
    const int segs = (W + RV - 1) / RV;
    const dim3 grid(blocks_of((long)D * H * segs)), block(kCclThreads);
    if (mode == CVX_MASK_LE) hipLaunchKernelGGL(k_mask_threshold<CVX_MASK_LE>, grid, block, 0, st, d2, ccl_dims(D, H, W), pad, threshold_d2, segs, out);
    else hipLaunchKernelGGL(k_mask_threshold<CVX_MASK_GT>, grid, block, 0, st, d2, ccl_dims(D, H, W), pad, threshold_d2, segs, out);
    return cvx_check_launch();
}

extern "C" int cvx_mask_added_voxels(const int32_t* labels, const uint8_t* before, int D, int H, int W, long k, int64_t* out, hipStream_t st) {
    long n = 0;
    if (const char* why = extents_fault(D, H, W, kExtentAny, n)) return cvx_fail("mask_added_voxels", why);
    if (k < 0) return cvx_fail("mask_added_voxels", "k < 0");
    if (!rows_fit(k, 1)) return cvx_fail("mask_added_voxels", "k rows do not fit in memory");
    if (k == 0) return 0;
    if (!out || (n > 0 && (!labels || !before))) return cvx_fail("mask_added_voxels", "null pointer");
    if (((uintptr_t)out & 7) || ((uintptr_t)labels & 3)) return cvx_fail("mask_added_voxels", "misaligned pointer");
    CVX_HIP(hipMemsetAsync(out, 0, (size_t)k * sizeof(int64_t), st));
    if (n == 0) return 0;
    const Dims d = ccl_dims(D, H, W);
    hipLaunchKernelGGL(k_mask_added, dim3((unsigned)tile_count(d)), dim3(kCclThreads), 0, st, labels, before, (long long*)out, d, clamp_int(k));
    return cvx_check_launch();
}
