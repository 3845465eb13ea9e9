// Mean curvature of the surface of labels > 0 by the ball-volume integral invariant (`--curvature`): the fraction of a ball of
// radius r, centred on the surface, that lies inside the object is 1/2 - (3/16) r H.  The definition (the ball, the surface, the
// scored band, the pairing of a surface voxel with its background face neighbours, the integer formula of h) is in
// include/cryovit_hip.h.  Integers only, no atomics in the map, so two calls give the same bits.
//
// THE MAP.  n(v) = the foreground voxels under the ball at v is needed on a two-voxel shell only: the scored surface voxels p and
// their background face neighbours q.
//   k_curv_pack   F = labels > 0 as bits, one uint64 per 64 voxels of a row ([D][H][WW], bit i of word w = voxel x = 64 w + i;
//                 bits past W are 0; bit_rows.h): one wave per word, one __ballot.
//   k_curv_map    one workgroup per 4x8x64 output tile.
//     1. the rows of the tile with a halo of one row and one word go to LDS; 32 threads form the word of scored surface voxels
//        of the tile's 32 rows with shifts and ANDs.  A tile without one stores CURV_NONE and is done: most tiles end here.
//     2. the rest of the halo: r + 1 rows in z and y (the ball at a q one voxel outside the tile), still one word on each side
//        in x (r + 1 <= 64): (6 + 2r)(10 + 2r) rows of 3 words, 7.7 KB at r = 5, 38.3 KB at r = 16 (dynamic LDS).
//     3. the shell voxels of the tile and of the one-voxel frame around it are compacted into an LDS queue in raster order:
//        one need word per row of the frame, a prefix sum over the 60 rows, slot = prefix + popcount(bits below).  No atomics.
//     4. a lane takes a queued voxel and sums popcount(row bits & span) over the (dz, dy) of the ball, whose half-widths
//        w(dz, dy) come with the kernel arguments (the loop is the same for every lane, so the table is read by scalar loads):
//        at most (2r + 1)^2 popcounts per voxel and no loop along x.  The 2w + 1 <= 33 bits of a span lie in at most two of the
//        row's three words.  n goes to a uint16 LDS array over the frame (N <= 17077).
//     5. one lane per x, one wave per z: h from n(p) and the n(q) in LDS; the tile leaves with plain coalesced stores.
//   Static LDS 16.3 KB; with the rows 24 KB at r = 5 and 54.6 KB at r = 16.
// A q on the frame is also computed by the tile it lies in when that one needs it: the price of no n volume in global memory.
//
// THE TABLE.  k_curv_stats reads labels with the one-voxel halo of voxel_rows.h (a surface voxel without a score is found by its
// neighbours) and h directly, and reduces per id by table_reduce of voxel_rows.h: thread, wave with a single id, the waves of a
// workgroup that hold the same id, then 64-bit integer atomics.  min and max start from +-2^62 and are set to 0 by k_curv_stats_fin for an
// id without a scored voxel.
#include "bit_rows.h"

namespace cvx {

constexpr int kCurvRmin = CVX_CURVATURE_RADIUS_MIN, kCurvRmax = CVX_CURVATURE_RADIUS_MAX;
constexpr int EZ = TZ + 2, EY = TY + 2, EX = TX + 2;  // the frame: the tile and one voxel around it
constexpr int kFrameRows = EZ * EY;                   // 60
constexpr int kFrameCells = kFrameRows * EX;          // 3960
constexpr int kCurvQueue = TZ * TY * EX + 2 * TY * TX + 2 * TZ * TX;  // own rows with both x neighbours + the four faces: 3648
static_assert(kFrameCells < 65536, "a frame cell fits in a uint16");

// the ball |o|^2 <= r^2 as half-widths along x: hw[|dz|][|dy|] for |dy| <= ymax[|dz|]; N voxels
struct Ball {
    int r, N;
    signed char ymax[kCurvRmax + 1];
    signed char hw[kCurvRmax + 1][kCurvRmax + 1];
};

inline Ball make_ball(int r) {
    Ball b{};
    b.r = r;
    for (int dz = 0; dz <= r; ++dz) {
        int ym = 0;
        for (int dy = 0; dy <= r; ++dy) {
            const int w = ball_half_width(r * r, dz, dy);
            if (w >= 0) {
                ym = dy;
                b.N += (2 * w + 1) * (dz ? 2 : 1) * (dy ? 2 : 1);
            }
            b.hw[dz][dy] = (signed char)w;
        }
        b.ymax[dz] = (signed char)ym;
    }
    return b;
}

// one wave per word
__global__ __launch_bounds__(kCclThreads) void k_curv_pack(const int* __restrict__ labels, BitDims d, long words, Word* __restrict__ bits) {
    long g, row;
    int x;
    if (!wave_word(d.WW, words, g, row, x)) return;
    const Word f = __ballot(x < d.W && labels[row * d.W + x] > 0);
    if ((threadIdx.x & 63) == 0) bits[g] = f;
}

__global__ __launch_bounds__(kCclThreads) void k_curv_fill(int* __restrict__ h, long n) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i < n) h[i] = CVX_CURV_NONE;
}

__global__ __launch_bounds__(kCclThreads) void k_curv_map(const Word* __restrict__ bits, BitDims d, Ball ball, int* __restrict__ h) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    static_assert(kCclThreads >= kFrameRows && kCclThreads >= TZ * TY, "one thread per row of the frame");
    extern __shared__ Word rows[];  // [TZ + 2 R1][TY + 2 R1][3]: the rows from (z0 - R1, y0 - R1), the words x0 / 64 - 1 .. + 1
    __shared__ unsigned short n_of[kFrameCells];
    __shared__ unsigned short queue[kCurvQueue];
    __shared__ Word scored[TZ * TY];   // per own row: the scored surface voxels
    __shared__ Word need[kFrameRows];  // per frame row: the voxels x0 .. x0 + 63 whose n is needed
    __shared__ int need_side[kFrameRows];  // bit 0: x0 - 1 is needed, bit 1: x0 + 64
    __shared__ int first[kFrameRows + 1];  // the queue slot of a frame row's first voxel; [kFrameRows]: the queue's length
    const int r = ball.r, R1 = r + 1;
    const int HY = TY + 2 * R1, HZ = TZ + 2 * R1;
    const int b = blockIdx.x;
    const int x0 = (b % d.tx) * TX, y0 = (b / d.tx % d.ty) * TY, z0 = (b / d.tx / d.ty) * TZ;
    const int w0 = x0 / 64 - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // rows[(zz * HY + yy) * 3 + w] of the frame rows (near) or of all the others; a word outside the volume is 0
    auto load = [&](bool near) {
        for (int c = threadIdx.x; c < HZ * HY * 3; c += kCclThreads) {
            const int w = c % 3, yy = c / 3 % HY, zz = c / (3 * HY);
            if (near != (zz >= r && zz < r + EZ && yy >= r && yy < r + EY)) continue;
            const int gw = w0 + w, y = y0 - R1 + yy, z = z0 - R1 + zz;
            const bool in = (unsigned)gw < (unsigned)d.WW && (unsigned)y < (unsigned)d.H && (unsigned)z < (unsigned)d.D;
            rows[c] = in ? bits[((long)z * d.H + y) * d.WW + gw] : 0;
        }
    };
    // the three words of the row (oz, oy) in tile coordinates, -1 - r <= oz < TZ + 1 + r etc.
    auto row_at = [&](int oz, int oy) { return rows + ((oz + R1) * HY + oy + R1) * 3; };
    load(true);
    __syncthreads();
    int any = 0;
    if (threadIdx.x < TZ * TY) {
        const int oz = threadIdx.x / TY, oy = threadIdx.x % TY;
        const int z = z0 + oz, y = y0 + oy;
        const Word* c = row_at(oz, oy);
        // a neighbour outside the volume is no background
        const Word up = z > 0 ? row_at(oz - 1, oy)[1] : ~0ull, down = z + 1 < d.D ? row_at(oz + 1, oy)[1] : ~0ull;
        const Word front = y > 0 ? row_at(oz, oy - 1)[1] : ~0ull, back = y + 1 < d.H ? row_at(oz, oy + 1)[1] : ~0ull;
        const int last = d.W - 1 - x0;  // the bit of the volume's last voxel of the row, if below 64
        const Word left = c[1] << 1 | c[0] >> 63 | (x0 == 0 ? 1ull : 0ull);
        const Word right = c[1] >> 1 | c[2] << 63 | (last < 64 ? ~0ull << last : 0ull);
        const Word surface = c[1] & ~(up & down & front & back & left & right);
        // scored: r + 1 <= index <= extent - r - 2 on every axis
        const int lo = max(0, R1 - x0), hi = min(63, d.W - r - 2 - x0);
        Word band = 0;
        if (z >= R1 && z <= d.D - r - 2 && y >= R1 && y <= d.H - r - 2 && lo <= hi) band = (~0ull >> (63 - hi)) & (~0ull << lo);
        const Word s = surface & band;
        scored[threadIdx.x] = s;
        any = s != 0;
    }
    const int z = z0 + wave, x = x0 + lane;
    if (!__syncthreads_or(any)) {  // no scored voxel in this tile
        if (z < d.D && x < d.W)
            for (int yy = 0; yy < TY && y0 + yy < d.H; ++yy) h[((long)z * d.H + y0 + yy) * d.W + x] = CVX_CURV_NONE;
        return;
    }
    load(false);
    // what is needed of every frame row: the scored voxels and their background face neighbours
    if (threadIdx.x < kFrameRows) {
        const int oz = threadIdx.x / EY - 1, oy = threadIdx.x % EY - 1;
        const bool zin = oz >= 0 && oz < TZ, yin = oy >= 0 && oy < TY;
        auto sc = [&](int a, int c) { return a >= 0 && a < TZ && c >= 0 && c < TY ? scored[a * TY + c] : 0ull; };
        Word nd = 0;
        int side = 0;
        if (zin || yin) {  // not one of the frame's edge rows, which touch no own voxel by a face
            const Word* c = row_at(oz, oy);  // a frame row: loaded before the first barrier
            const Word s = sc(oz, oy);
            const Word around = sc(oz - 1, oy) | sc(oz + 1, oy) | sc(oz, oy - 1) | sc(oz, oy + 1) | s << 1 | s >> 1;
            nd = s | (~c[1] & around);
            side = (int)((s & 1) && !(c[0] >> 63)) | (int)((s >> 63) && !(c[2] & 1)) << 1;
        }
        need[threadIdx.x] = nd;
        need_side[threadIdx.x] = side;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int at = 0;
        for (int f = 0; f < kFrameRows; ++f) {
            first[f] = at;
            at += __popcll(need[f]) + (need_side[f] & 1) + (need_side[f] >> 1);
        }
        first[kFrameRows] = at;  // <= kCurvQueue: own rows give at most 66 each, the rows of the four faces 64, the others none
    }
    __syncthreads();
    for (int f = wave; f < kFrameRows; f += TZ) {
        const Word nd = need[f];
        const int side = need_side[f];
        int slot = first[f];
        if (lane == 0 && (side & 1)) queue[slot] = (unsigned short)(f * EX);
        slot += side & 1;
        if (nd >> lane & 1) queue[queue_slot(slot, nd, lane)] = (unsigned short)(f * EX + 1 + lane);
        if (lane == 0 && (side & 2)) queue[slot + __popcll(nd)] = (unsigned short)(f * EX + EX - 1);
    }
    __syncthreads();
    // n of the queued voxels: the row (ez - 1 + dz, ey - 1 + dy) of the tile, the bits ex - 1 - w .. ex - 1 + w of its middle word
    const int qn = first[kFrameRows];
    for (int i = threadIdx.x; i < qn; i += kCclThreads) {
        const int cell = queue[i];
        const int ex = cell % EX, ey = cell / EX % EY, ez = cell / (EX * EY);
        const Word* centre = row_at(ez - 1, ey - 1);
        const int xb = 64 + ex - 1;  // the bit of the voxel among the 192 of its row: 63 .. 128
        int n = 0;
        for (int dz = -r; dz <= r; ++dz) {
            const int az = dz < 0 ? -dz : dz, ym = ball.ymax[az];
            for (int dy = -ym; dy <= ym; ++dy) {
                const int w = ball.hw[az][dy < 0 ? -dy : dy];
                n += __popcll(row_span(centre + (dz * HY + dy) * 3, 3, xb - w, w));  // 47 <= xb - w <= 128, xb + w <= 144
            }
        }
        n_of[cell] = (unsigned short)n;
    }
    __syncthreads();
    if (z >= d.D || x >= d.W) return;
    for (int yy = 0; yy < TY && y0 + yy < d.H; ++yy) {
        int out = CVX_CURV_NONE;
        if (scored[wave * TY + yy] >> lane & 1) {
            const int cell = ((wave + 1) * EY + yy + 1) * EX + lane + 1;
            // every neighbour of a scored voxel is inside the volume
            const Word* c = row_at(wave, yy);
            const bool bg[6] = {!(row_at(wave - 1, yy)[1] >> lane & 1), !(row_at(wave + 1, yy)[1] >> lane & 1),
                                !(row_at(wave, yy - 1)[1] >> lane & 1), !(row_at(wave, yy + 1)[1] >> lane & 1),
                                !(lane ? c[1] >> (lane - 1) & 1 : c[0] >> 63), !(lane < 63 ? c[1] >> (lane + 1) & 1 : c[2] & 1)};
            const int step[6] = {-EY * EX, EY * EX, -EX, EX, -1, 1};
            long long m = 0, S = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q)
                if (bg[q]) {
                    m += 1;
                    S += n_of[cell + step[q]];
                }
            // m >= 1: the voxel is a surface voxel
            const long long num = 32768ll * (m * ball.N - m * n_of[cell] - S), den = 3ll * r * m * ball.N;
            long long q = num / den;
            if (num % den != 0 && num < 0) q -= 1;  // towards minus infinity
            out = (int)q;
        }
        h[((long)z * d.H + y0 + yy) * d.W + x] = out;
    }
}

// ---- the per-instance table ----

constexpr long long kCurvFar = 1ll << 62;

__global__ __launch_bounds__(kCclThreads) void k_curv_stats_init(long long* __restrict__ out, long cells) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i < cells) out[i] = i % CVX_CURVATURE_COLS == 3 ? kCurvFar : i % CVX_CURVATURE_COLS == 4 ? -kCurvFar : 0;
}

__global__ __launch_bounds__(kCclThreads) void k_curv_stats_fin(long long* __restrict__ out, long k) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i < k && out[i * CVX_CURVATURE_COLS] == 0) out[i * CVX_CURVATURE_COLS + 3] = out[i * CVX_CURVATURE_COLS + 4] = 0;
}

struct CurvAcc {
    long long n, sum, sum2, convex, unscored;
    int lo, hi;
    __device__ void wave_combine() {
        n = wave_sum(n), sum = wave_sum(sum), sum2 = wave_sum(sum2), convex = wave_sum(convex), unscored = wave_sum(unscored);
        lo = wave_min(lo), hi = wave_max(hi);
    }
    __device__ void merge(const CurvAcc& a) {
        n += a.n, sum += a.sum, sum2 += a.sum2, convex += a.convex, unscored += a.unscored;
        lo = min(lo, a.lo), hi = max(hi, a.hi);
    }
};
constexpr CurvAcc kCurvEmpty{0, 0, 0, 0, 0, INT_MAX, INT_MIN};

// acc goes to row id - 1; acc = empty
__device__ __forceinline__ void curv_flush(long long* __restrict__ out, int id, CurvAcc& acc) {
    long long* row = out + (long)(id - 1) * CVX_CURVATURE_COLS;
    auto* u = (unsigned long long*)row;
    if (acc.n) {
        atomicAdd(u + 0, (unsigned long long)acc.n);
        atomicAdd(u + 1, (unsigned long long)acc.sum);  // a negative sum wraps to the right one
        atomicAdd(u + 2, (unsigned long long)acc.sum2);
        table_min(row + 3, acc.lo);
        table_max(row + 4, acc.hi);
        if (acc.convex) atomicAdd(u + 5, (unsigned long long)acc.convex);
    }
    if (acc.unscored) atomicAdd(u + 6, (unsigned long long)acc.unscored);
    acc = kCurvEmpty;
}

__global__ __launch_bounds__(kCclThreads) void k_curv_stats(const int* __restrict__ labels, const int* __restrict__ h,
                                                            long long* __restrict__ out, Dims d, int k) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    __shared__ int ids[kHaloCells];
    int z0, y0, x0;
    tile_origin(d, z0, y0, x0);
    tile_load_ids(labels, d, z0, y0, x0, INT_MAX, ids);  // every positive label is foreground, whatever k
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int z = z0 + wave, x = x0 + lane;
    CurvAcc acc = kCurvEmpty;
    int cur = 0;  // the id acc belongs to; 0: none yet
    if (z < d.D && x < d.W)
        for (int yy = 0; yy < TY && y0 + yy < d.H; ++yy) {
            const int y = y0 + yy, c = halo_cell(wave, yy, lane);
            const int id = ids[c];
            if (id < 1 || id > k) continue;
            const int v = h[((long)z * d.H + y) * d.W + x];
            bool unscored = false;
            if (v == CVX_CURV_NONE) {  // a surface voxel?  A cell outside the volume reads 0: only neighbours inside count
                unscored = (z > 0 && !ids[c - kHaloY * kHaloX]) || (z + 1 < d.D && !ids[c + kHaloY * kHaloX]) ||
                           (y > 0 && !ids[c - kHaloX]) || (y + 1 < d.H && !ids[c + kHaloX]) || (x > 0 && !ids[c - 1]) ||
                           (x + 1 < d.W && !ids[c + 1]);
                if (!unscored) continue;
            }
            if (id != cur) {
                if (cur) curv_flush(out, cur, acc);
                cur = id;
            }
            if (unscored) {
                acc.unscored += 1;
                continue;
            }
            acc.n += 1;
            acc.sum += v;
            acc.sum2 += (long long)v * v;
            acc.convex += v > 0;
            acc.lo = min(acc.lo, v);
            acc.hi = max(acc.hi, v);
        }
    table_reduce(acc, cur, [&](int id, CurvAcc& a) { curv_flush(out, id, a); });
}

}  // namespace cvx

using namespace cvx;

extern "C" long cvx_curvature_workspace_bytes(int D, int H, int W) { return bitmap_workspace_bytes(D, H, W); }

extern "C" int cvx_curvature_map(const int32_t* labels, int D, int H, int W, int radius, int32_t* h, void* workspace, long workspace_bytes,
                                 hipStream_t st) {
    long n = 0;
    if (const char* why = extents_fault(D, H, W, kExtentMax, n)) return cvx_fail("curvature_map", why);
    if (radius < kCurvRmin || radius > kCurvRmax) return cvx_fail("curvature_map", "radius must lie in [2, 16]");
    if (n == 0) return 0;
    if (!labels || !h || !workspace) return cvx_fail("curvature_map", "null pointer");
    if ((((uintptr_t)labels | (uintptr_t)h) & 3) || ((uintptr_t)workspace & 7)) return cvx_fail("curvature_map", "misaligned pointer");
    const BitDims d = bit_dims(D, H, W);
    if (workspace_bytes < bitmap_bytes(d)) return cvx_fail("curvature_map", "workspace shorter than cvx_curvature_workspace_bytes");
    if (labels == h) return cvx_fail("curvature_map", "labels and h must be different arrays");
    const int least = 2 * radius + 3;  // below it no index satisfies r + 1 <= i <= extent - r - 2
    if (D < least || H < least || W < least) {
        hipLaunchKernelGGL(k_curv_fill, dim3(blocks_of(n)), dim3(kCclThreads), 0, st, h, n);
        return cvx_check_launch();
    }
    const long words = bitmap_words(d);
    hipLaunchKernelGGL(k_curv_pack, dim3(wave_blocks_of(words)), dim3(kCclThreads), 0, st, labels, d, words, (Word*)workspace);
    if (const int rc = cvx_check_launch()) return rc;
    const Ball ball = make_ball(radius);
    const size_t lds = (size_t)(TZ + 2 * (radius + 1)) * (TY + 2 * (radius + 1)) * 3 * sizeof(Word);
    hipLaunchKernelGGL(k_curv_map, dim3((unsigned)tile_count(ccl_dims(D, H, W))), dim3(kCclThreads), lds, st, (const Word*)workspace, d, ball, h);
    return cvx_check_launch();
}

extern "C" int cvx_curvature_stats(const int32_t* labels, const int32_t* h, int D, int H, int W, long k, int64_t* table, hipStream_t st) {
    long n = 0;
    if (const char* why = extents_fault(D, H, W, kExtentMax, n)) return cvx_fail("curvature_stats", why);
    if (k < 0) return cvx_fail("curvature_stats", "k < 0");
    if (!rows_fit(k, CVX_CURVATURE_COLS)) return cvx_fail("curvature_stats", "k rows do not fit in memory");
    if (k == 0) return 0;
    if (!table || (n > 0 && (!labels || !h))) return cvx_fail("curvature_stats", "null pointer");
    if (((uintptr_t)table & 7) || (((uintptr_t)labels | (uintptr_t)h) & 3)) return cvx_fail("curvature_stats", "misaligned pointer");
    const long cells = k * CVX_CURVATURE_COLS;
    if ((cells + kCclThreads - 1) / kCclThreads > INT_MAX) return cvx_fail("curvature_stats", "k rows do not fit in one launch");
    hipLaunchKernelGGL(k_curv_stats_init, dim3(blocks_of(cells)), dim3(kCclThreads), 0, st, (long long*)table, cells);
    if (const int rc = cvx_check_launch()) return rc;
    if (n > 0) {
        const Dims d = ccl_dims(D, H, W);
        hipLaunchKernelGGL(k_curv_stats, dim3((unsigned)tile_count(d)), dim3(kCclThreads), 0, st, labels, h, (long long*)table, d, clamp_int(k));
        if (const int rc = cvx_check_launch()) return rc;
    }
    hipLaunchKernelGGL(k_curv_stats_fin, dim3(blocks_of(k)), dim3(kCclThreads), 0, st, (long long*)table, k);
    return cvx_check_launch();
}
