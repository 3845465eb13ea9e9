// Membrane picking (`--pick`): evenly spaced surface voxels of every instance with the membrane normal, the particle positions of
// subtomogram averaging.  The definition (candidate, key, the lexicographically first maximal independent set, the moment M of the
// ball, the pick table) is in include/cryovit_hip.h.  Integers only and no atomics (a round's "changed" flag is a plain store of 1), so
// two calls give the same bits.
//
// PACK.  k_pick_pack: F = labels > 0 and "the label lies in 1..k" as bits, one uint64 per 64 voxels of a row ([D][H][WW], bit i of
//   word w = voxel x = 64 w + i; bits past W are 0; bit_rows.h): one wave per word, two __ballots.  k_pick_cand: one thread per word
//   turns the second bitmap into the candidates with shifts and ANDs of F's words: surface, the band r <= index <= extent - 1 - r.
//   The state of the selection is a pair of bitmaps [2][D][H][WW]: undecided (the candidates at the start) and picked (empty).
//
// SELECTION.  k_pick_round, one workgroup per 4x8x64 tile, one round: an undecided voxel p is rejected when a picked voxel conflicts
//   with it (same id, squared distance < s^2), picked when no undecided conflicting voxel has a smaller key, and waits otherwise.
//   A round reads the state the round before left and writes ANOTHER one (ping-pong): a voxel that read `picked` before and
//   `undecided` after a neighbour's in-place update would see neither bit and be picked wrongly.  The fixpoint is the greedy set.
//     1. 32 threads read the tile's own 32 words of both bitmaps.  A tile without an undecided voxel copies them and is done.
//     2. both bitmaps with a halo of s - 1 rows and one word go to LDS: (4 + 2(s-1))(8 + 2(s-1)) rows of 3 words each, 31 KB per
//        bitmap at s = 16; words outside the volume are 0.
//     3. the undecided voxels of the tile are compacted into an LDS queue in raster order (a prefix sum over the 32 rows, slot =
//        prefix + popcount(bits below)).
//     4. a lane takes a queued voxel and walks the (dz, dy) rows of the open ball |o|^2 < s^2, whose half-widths lie in LDS; per row
//        it iterates over the set bits of `row & span` only.  A label is read, and a key computed, only for a set bit.  First the
//        picked rows (skipped while the tile sees no picked voxel at all: the first round), then the undecided ones, leaving on the
//        first smaller key.
//     5. a wave per row gathers the decisions with two __ballots; the tile's 32 words of both bitmaps leave by plain stores.
// EMIT.  k_pick_count: picks per row; k_pick_scan: one workgroup, exclusive prefix sums in row order and the total P (the host
//   reads it once); k_pick_place: one thread per word writes z, y, x, id of its picks at row base + popcount(bits before);
//   k_pick_moments: one wave per pick, lanes over the (dz, dy) rows of the ball |o|^2 <= r^2: dz * popcount, dy * popcount and the
//   x-moment of the set bits of `row & span` from six masked popcounts; a wave sum, plain stores.
#include "bit_rows.h"

namespace cvx {

constexpr int kPickRmin = CVX_PICK_RADIUS_MIN, kPickRmax = CVX_PICK_RADIUS_MAX;
constexpr int kPickSmin = CVX_PICK_SPACING_MIN, kPickSmax = CVX_PICK_SPACING_MAX;
constexpr int kPickRows = TZ * TY;  // 32 rows of one word per tile
constexpr int kPickScanThreads = 1024, kPickScanPer = 4;
constexpr int kPickHw = kPickSmax;  // half-width table [kPickHw][kPickHw]: |dz|, |dy| <= s - 1

// murmur3's finaliser
__device__ __forceinline__ unsigned fmix32(unsigned h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// one wave per word
__global__ __launch_bounds__(kCclThreads) void k_pick_pack(const int* __restrict__ labels, BitDims d, long words, int k, Word* __restrict__ fg,
                                                           Word* __restrict__ state) {
    long g, row;
    int x;
    if (!wave_word(d.WW, words, g, row, x)) return;
    const int l = x < d.W ? labels[row * d.W + x] : 0;
    const Word f = __ballot(l > 0), ok = __ballot(l >= 1 && l <= k);
    if ((threadIdx.x & 63) == 0) {
        fg[g] = f;
        state[g] = ok;
        state[words + g] = 0;
    }
}

// state[g] = the candidates among the voxels with an id: one thread per word, in place (only F's words of other rows are read)
__global__ __launch_bounds__(kCclThreads) void k_pick_cand(const Word* __restrict__ fg, BitDims d, long words, int r, Word* __restrict__ state) {
    const long g = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (g >= words) return;
    const Word ok = state[g];
    if (!ok) return;
    const int w = (int)(g % d.WW), y = (int)(g / d.WW % d.H), z = (int)(g / d.WW / d.H);
    const int lo = max(0, r - 64 * w), hi = min(63, d.W - 1 - r - 64 * w);
    Word cand = 0;
    if (z >= r && z <= d.D - 1 - r && y >= r && y <= d.H - 1 - r && lo <= hi) {  // r >= 1: every face neighbour of a band voxel is inside
        const long sy = d.WW, sz = (long)d.H * d.WW;
        const Word c = fg[g];
        const Word left = c << 1 | (w > 0 ? fg[g - 1] >> 63 : 0ull), right = c >> 1 | (w + 1 < d.WW ? fg[g + 1] << 63 : 0ull);
        const Word inner = fg[g - sz] & fg[g + sz] & fg[g - sy] & fg[g + sy] & left & right;
        cand = ok & c & ~inner & (~0ull >> (63 - hi)) & (~0ull << lo);
    }
    state[g] = cand;
}

// the dynamic LDS of k_pick_round, in bytes, every part a multiple of 16
__host__ __device__ constexpr int pick_round_rows(int s) { return (TZ + 2 * (s - 1)) * (TY + 2 * (s - 1)) * 3; }
constexpr int kPickLdsFixed = 2 * kPickRows * (int)sizeof(Word) + 48 * (int)sizeof(int) + kPickHw * kPickHw + kTileVox * (int)sizeof(unsigned short);
__host__ __device__ constexpr int pick_round_lds(int s) { return 2 * pick_round_rows(s) * (int)sizeof(Word) + kPickLdsFixed; }

__global__ __launch_bounds__(kCclThreads) void k_pick_round(const int* __restrict__ labels, const Word* __restrict__ in, Word* __restrict__ out,
                                                            BitDims d, long words, int s, unsigned seed, int* __restrict__ changed) {
    static_assert(kCclThreads == TZ * TX && TX == 64, "one wave per z plane of the tile, one lane per x");
    static_assert(kCclThreads >= kPickHw * kPickHw && kTileVox < (1 << 14), "one thread per table entry; a cell and a decision fit in a uint16");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int S1 = s - 1, HY = TY + 2 * S1, HZ = TZ + 2 * S1, nrows = HZ * HY * 3;
    Word* und = (Word*)lds;                   // [HZ][HY][3]: the rows from (z0 - S1, y0 - S1), the words x0 / 64 - 1 .. + 1
    Word* pic = und + nrows;                  // the same of picked
    Word* own_u = pic + nrows;                // [32]
    Word* own_p = own_u + kPickRows;          // [32]
    int* first = (int*)(own_p + kPickRows);   // [33] of 48: the queue slot of a row's first voxel; [32]: the queue's length
    signed char* hw = (signed char*)(first + 48);                          // [kPickHw][kPickHw]
    unsigned short* queue = (unsigned short*)(hw + kPickHw * kPickHw);     // [2048]: cell | decision << 14
    const int b = blockIdx.x;
    const int x0 = (b % d.tx) * TX, y0 = (b / d.tx % d.ty) * TY, z0 = (b / d.tx / d.ty) * TZ;
    const int wx = x0 / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Word* in_u = in;
    const Word* in_p = in + words;
    const Word tail = tail_mask(d.W);  // a bit past W is never followed to a label, whatever the state holds
    // 1. the tile's own words
    long own_g = -1;
    Word u = 0, pk = 0;
    if (threadIdx.x < kPickRows) {
        const int z = z0 + threadIdx.x / TY, y = y0 + threadIdx.x % TY;
        if (z < d.D && y < d.H) {
            own_g = ((long)z * d.H + y) * d.WW + wx;
            const Word keep = wx == d.WW - 1 ? tail : ~0ull;
            u = in_u[own_g] & keep;
            pk = in_p[own_g] & keep;
        }
        own_u[threadIdx.x] = u;
        own_p[threadIdx.x] = pk;
    }
    if (!__syncthreads_or(u != 0)) {  // nothing to decide here
        if (own_g >= 0) {
            out[own_g] = 0;
            out[words + own_g] = pk;
        }
        return;
    }
    // 2. both bitmaps with their halo; a word outside the volume is 0
    int seen = 0;
    for (int c = threadIdx.x; c < nrows; c += kCclThreads) {
        const int w = c % 3, yy = c / 3 % HY, zz = c / (3 * HY);
        const int gw = wx - 1 + w, y = y0 - S1 + yy, z = z0 - S1 + zz;
        const bool inside = (unsigned)gw < (unsigned)d.WW && (unsigned)y < (unsigned)d.H && (unsigned)z < (unsigned)d.D;
        const long g = ((long)z * d.H + y) * d.WW + gw;
        const Word keep = gw == d.WW - 1 ? tail : ~0ull;
        const Word p = inside ? in_p[g] & keep : 0;
        und[c] = inside ? in_u[g] & keep : 0;
        pic[c] = p;
        seen |= p != 0;
    }
    if (threadIdx.x < kPickHw * kPickHw) hw[threadIdx.x] = (signed char)ball_half_width(s * s - 1, threadIdx.x / kPickHw, threadIdx.x % kPickHw);
    if (threadIdx.x == 0) {
        int at = 0;
        for (int f = 0; f < kPickRows; ++f) {
            first[f] = at;
            at += __popcll(own_u[f]);
        }
        first[kPickRows] = at;
    }
    const int any_picked = __syncthreads_or(seen);
    // 3. the queue
    for (int f = wave; f < kPickRows; f += TZ) {
        const Word m = own_u[f];
        if (m >> lane & 1) queue[queue_slot(first[f], m, lane)] = (unsigned short)(f * TX + lane);
    }
    __syncthreads();
    // 4. the decisions
    const int qn = first[kPickRows];
    int acted = 0;
    for (int i = threadIdx.x; i < qn; i += kCclThreads) {
        const int cell = queue[i];
        const int lx = cell % TX, oy = cell / TX % TY, oz = cell / (TX * TY);
        const int z = z0 + oz, y = y0 + oy, x = x0 + lx;
        const long idx = ((long)z * d.H + y) * d.W + x;
        const int id = labels[idx];
        const unsigned hash = fmix32((unsigned)idx ^ seed);
        const int centre = ((oz + S1) * HY + oy + S1) * 3, xb = 64 + lx;  // the bit of the voxel among the 192 of its row: 64 .. 127
        // does a set bit of v (the bits from `lo` of the row (z + dz, y + dy)) hold a conflicting voxel, `smaller`: with a smaller key?
        auto conflict = [&](Word v, int dz, int dy, int lo, bool smaller) {
            const long base = ((long)(z + dz) * d.H + y + dy) * d.W + x0 - 64 + lo;
            while (v) {
                const int j = __ffsll((long long)v) - 1;
                v &= v - 1;
                const long other = base + j;
                if (labels[other] != id) continue;
                if (!smaller) return true;
                const unsigned h = fmix32((unsigned)other ^ seed);
                if (h < hash || (h == hash && other < idx)) return true;
            }
            return false;
        };
        int decision = 2;  // picked, unless
        for (int pass = any_picked ? 0 : 1; pass < 2 && decision == 2; ++pass) {
            const Word* rows = pass ? und : pic;
            for (int dz = -S1; dz <= S1 && decision == 2; ++dz)
                for (int dy = -S1; dy <= S1; ++dy) {
                    const int w = hw[(dz < 0 ? -dz : dz) * kPickHw + (dy < 0 ? -dy : dy)];
                    if (w < 0) continue;
                    const int lo = xb - w;  // 49 <= lo, lo + 2w <= 142
                    Word v = row_span(rows + centre + (dz * HY + dy) * 3, 3, lo, w);
                    if (pass && dz == 0 && dy == 0) v &= ~(1ull << w);  // not itself
                    if (v && conflict(v, dz, dy, lo, pass != 0)) {
                        decision = pass ? 0 : 1;  // it waits : it is rejected
                        break;
                    }
                }
        }
        queue[i] = (unsigned short)(cell | decision << 14);
        acted |= decision;
    }
    if (__syncthreads_or(acted) && threadIdx.x == 0) *changed = 1;
    // 5. the new words
    for (int f = wave; f < kPickRows; f += TZ) {
        const Word m = own_u[f];
        int decision = 0;
        if (m >> lane & 1) decision = queue[queue_slot(first[f], m, lane)] >> 14;
        const Word gone = __ballot(decision != 0), taken = __ballot(decision == 2);
        const int z = z0 + f / TY, y = y0 + f % TY;
        if (lane == 0 && z < d.D && y < d.H) {
            const long g = ((long)z * d.H + y) * d.WW + wx;
            out[g] = m & ~gone;
            out[words + g] = own_p[f] | taken;
        }
    }
}

// ---- emit ----

__global__ __launch_bounds__(kCclThreads) void k_pick_count(const Word* __restrict__ picked, long rows, int WW, int* __restrict__ row_first) {
    const long r = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (r >= rows) return;
    int n = 0;
    for (int w = 0; w < WW; ++w) n += __popcll(picked[r * WW + w]);
    row_first[r] = n;
}

// a[i] = the sum of a[0..i), in place; total = the sum (below 2^31: a pick is a voxel)
__global__ __launch_bounds__(kPickScanThreads) void k_pick_scan(int* __restrict__ a, long n, long long* __restrict__ total) {
    constexpr int kWaves = kPickScanThreads / 64;
    __shared__ int wsum[kWaves];
    const int wave = threadIdx.x >> 6;
    long long carry = 0;
    for (long base = 0; base < n; base += kPickScanThreads * kPickScanPer) {
        const long i0 = base + (long)threadIdx.x * kPickScanPer;
        int v[kPickScanPer], sv = 0;
#pragma unroll
        for (int j = 0; j < kPickScanPer; ++j) {
            v[j] = i0 + j < n ? a[i0 + j] : 0;
            sv += v[j];
        }
        const int incl = wave_scan_incl(sv);
        if ((threadIdx.x & 63) == 63) wsum[wave] = incl;
        __syncthreads();
        int woff = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int t = wsum[w];
            if (w < wave) woff += t;
            all += t;
        }
        long long run = carry + woff + incl - sv;
#pragma unroll
        for (int j = 0; j < kPickScanPer; ++j)
            if (i0 + j < n) {
                a[i0 + j] = (int)run;
                run += v[j];
            }
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// z, y, x, id of every pick: one thread per word
__global__ __launch_bounds__(kCclThreads) void k_pick_place(const int* __restrict__ labels, const Word* __restrict__ picked, BitDims d, long words,
                                                            const int* __restrict__ row_first, long P, int* __restrict__ table) {
    const long g = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (g >= words) return;
    const int w = (int)(g % d.WW);
    Word v = picked[g];
    if (w == d.WW - 1) v &= tail_mask(d.W);  // a bit past W is no voxel, whatever the state holds
    if (!v) return;
    const long row = g / d.WW;
    long slot = row_first[row];
    for (int u = 0; u < w; ++u) slot += __popcll(picked[g - w + u]);
    const int y = (int)(row % d.H), z = (int)(row / d.H);
    while (v) {
        const int x = 64 * w + __ffsll((long long)v) - 1;
        v &= v - 1;
        if (slot >= P) return;  // a P that is not this state's count: write nothing past the table
        int* t = table + slot * CVX_PICK_COLS;
        t[0] = z, t[1] = y, t[2] = x, t[3] = labels[row * d.W + x];
        ++slot;
    }
}

// M and n of every pick: one wave per pick
__global__ __launch_bounds__(kCclThreads) void k_pick_moments(const Word* __restrict__ fg, BitDims d, int r, long P, int* __restrict__ table) {
    const int lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * (kCclThreads / 64) + (threadIdx.x >> 6);
    if (p >= P) return;  // the whole wave alike
    int* t = table + p * CVX_PICK_COLS;
    const int z = t[0], y = t[1], x = t[2];
    int mz = 0, my = 0, mx = 0, n = 0;
    // a pick is a candidate: r <= index <= extent - 1 - r on every axis, so no row and no span leaves the volume
    const bool inside = z >= r && z <= d.D - 1 - r && y >= r && y <= d.H - 1 - r && x >= r && x <= d.W - 1 - r;
    const int side = 2 * r + 1;
    for (int c = lane; inside && c < side * side; c += 64) {
        const int dz = c / side - r, dy = c % side - r;
        const int w = ball_half_width(r * r, dz < 0 ? -dz : dz, dy < 0 ? -dy : dy);
        if (w < 0) continue;
        const Word v = row_span(fg + ((long)(z + dz) * d.H + y + dy) * d.WW, d.WW, x - w, w);  // bit j: dx = j - w
        const int cnt = __popcll(v);
        const int sj = __popcll(v & 0xaaaaaaaaaaaaaaaaull) + 2 * __popcll(v & 0xccccccccccccccccull) + 4 * __popcll(v & 0xf0f0f0f0f0f0f0f0ull) +
                       8 * __popcll(v & 0xff00ff00ff00ff00ull) + 16 * __popcll(v & 0xffff0000ffff0000ull) + 32 * __popcll(v & 0xffffffff00000000ull);
        n += cnt;
        mz += dz * cnt;
        my += dy * cnt;
        mx += sj - w * cnt;
    }
    mz = wave_sum(mz), my = wave_sum(my), mx = wave_sum(mx), n = wave_sum(n);
    if (lane == 0) t[4] = mz, t[5] = my, t[6] = mx, t[7] = n;
}

}  // namespace cvx

using namespace cvx;

namespace {

constexpr int kNoOption = INT_MIN;  // for pick_fault: the entry has no such argument

// what every entry refuses about the volume and the options it takes.  nullptr: fine
const char* pick_fault(int D, int H, int W, int radius, int spacing, long k, long& n) {
    if (const char* why = extents_fault(D, H, W, kExtentMax, n)) return why;
    if (radius != kNoOption && (radius < kPickRmin || radius > kPickRmax)) return "radius must lie in [2, 16]";
    if (spacing != kNoOption && (spacing < kPickSmin || spacing > kPickSmax)) return "spacing must lie in [2, 16]";
    if (k < 0) return "k < 0";
    return nullptr;
}

}  // namespace

extern "C" long cvx_pick_workspace_bytes(int D, int H, int W) { return bitmap_workspace_bytes(D, H, W); }

extern "C" int cvx_pick_pack(const int32_t* labels, int D, int H, int W, long k, int radius, uint64_t* fg, uint64_t* state, long workspace_bytes,
                             hipStream_t st) {
    long n = 0;
    if (const char* why = pick_fault(D, H, W, radius, kNoOption, k, n)) return cvx_fail("pick_pack", why);
    if (n == 0 || k == 0) return 0;
    if (!labels || !fg || !state) return cvx_fail("pick_pack", "null pointer");
    if (((uintptr_t)labels & 3) || (((uintptr_t)fg | (uintptr_t)state) & 7)) return cvx_fail("pick_pack", "misaligned pointer");
    const BitDims d = bit_dims(D, H, W);
    if (workspace_bytes < bitmap_bytes(d)) return cvx_fail("pick_pack", "workspace shorter than cvx_pick_workspace_bytes");
    const long words = bitmap_words(d);
    if (fg == state || fg == state + words) return cvx_fail("pick_pack", "fg and state must be different arrays");
    const int least = 2 * radius + 1;  // below it no index satisfies r <= i <= extent - 1 - r
    const bool none = D < least || H < least || W < least;
    hipLaunchKernelGGL(k_pick_pack, dim3(wave_blocks_of(words)), dim3(kCclThreads), 0, st, labels, d,
                       words, none ? 0 : clamp_int(k), (Word*)fg, (Word*)state);
    if (const int rc = cvx_check_launch()) return rc;
    if (none) return 0;
    hipLaunchKernelGGL(k_pick_cand, dim3(blocks_of(words)), dim3(kCclThreads), 0, st, (const Word*)fg, d, words, radius, (Word*)state);
    return cvx_check_launch();
}

extern "C" int cvx_pick_rounds(const int32_t* labels, int D, int H, int W, long k, int spacing, uint32_t seed, int rounds, uint64_t* state_a,
                               uint64_t* state_b, long workspace_bytes, int32_t* changed, hipStream_t st) {
    long n = 0;
    if (const char* why = pick_fault(D, H, W, kNoOption, spacing, k, n)) return cvx_fail("pick_rounds", why);
    if (rounds < 1) return cvx_fail("pick_rounds", "rounds < 1");
    if (!changed) return cvx_fail("pick_rounds", "null pointer");
    if ((uintptr_t)changed & 3) return cvx_fail("pick_rounds", "misaligned pointer");
    if (n > 0 && k > 0) {
        if (!labels || !state_a || !state_b) return cvx_fail("pick_rounds", "null pointer");
        if (((uintptr_t)labels & 3) || (((uintptr_t)state_a | (uintptr_t)state_b) & 7)) return cvx_fail("pick_rounds", "misaligned pointer");
        const long bytes = bitmap_bytes(bit_dims(D, H, W));
        if (workspace_bytes < bytes) return cvx_fail("pick_rounds", "workspace shorter than cvx_pick_workspace_bytes");
        const uintptr_t a = (uintptr_t)state_a, b = (uintptr_t)state_b;
        if (a < b + 2 * (uintptr_t)bytes && b < a + 2 * (uintptr_t)bytes) return cvx_fail("pick_rounds", "state_a and state_b must not overlap");
    }
    CVX_HIP(hipMemsetAsync(changed, 0, (size_t)rounds * sizeof(int), st));
    if (n == 0 || k == 0) return 0;
    const BitDims d = bit_dims(D, H, W);
    const long words = bitmap_words(d), tiles = tile_count(ccl_dims(D, H, W));
    CVX_HIP(hipFuncSetAttribute((const void*)k_pick_round, hipFuncAttributeMaxDynamicSharedMemorySize, pick_round_lds(kPickSmax)));
    for (int r = 0; r < rounds; ++r) {
        const Word* in = (const Word*)(r % 2 ? state_b : state_a);
        Word* out = (Word*)(r % 2 ? state_a : state_b);
        hipLaunchKernelGGL(k_pick_round, dim3((unsigned)tiles), dim3(kCclThreads), (size_t)pick_round_lds(spacing), st, labels, in, out, d, words,
                           spacing, (unsigned)seed, changed + r);
        if (const int rc = cvx_check_launch()) return rc;
    }
    return 0;
}

extern "C" int cvx_pick_count(const uint64_t* state, int D, int H, int W, long workspace_bytes, int32_t* row_first, int64_t* total, hipStream_t st) {
    long n = 0;
    if (const char* why = pick_fault(D, H, W, kNoOption, kNoOption, 0, n)) return cvx_fail("pick_count", why);
    if (!total) return cvx_fail("pick_count", "null pointer");
    if ((uintptr_t)total & 7) return cvx_fail("pick_count", "misaligned pointer");
    if (n == 0) {
        CVX_HIP(hipMemsetAsync(total, 0, sizeof(int64_t), st));
        return 0;
    }
    if (!state || !row_first) return cvx_fail("pick_count", "null pointer");
    if (((uintptr_t)state & 7) || ((uintptr_t)row_first & 3)) return cvx_fail("pick_count", "misaligned pointer");
    const BitDims d = bit_dims(D, H, W);
    if (workspace_bytes < bitmap_bytes(d)) return cvx_fail("pick_count", "workspace shorter than cvx_pick_workspace_bytes");
    const long rows = (long)D * H, words = rows * d.WW;
    hipLaunchKernelGGL(k_pick_count, dim3(blocks_of(rows)), dim3(kCclThreads), 0, st, (const Word*)state + words, rows, d.WW, row_first);
    if (const int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_pick_scan, dim3(1), dim3(kPickScanThreads), 0, st, row_first, rows, (long long*)total);
    return cvx_check_launch();
}

extern "C" int cvx_pick_emit(const int32_t* labels, const uint64_t* fg, const uint64_t* state, const int32_t* row_first, int D, int H, int W,
                             int radius, long workspace_bytes, long P, int32_t* table, hipStream_t st) {
    long n = 0;
    if (const char* why = pick_fault(D, H, W, radius, kNoOption, 0, n)) return cvx_fail("pick_emit", why);
    if (P < 0 || P > n) return cvx_fail("pick_emit", "P outside [0, D*H*W]");
    if (P == 0) return 0;
    if (!labels || !fg || !state || !row_first || !table) return cvx_fail("pick_emit", "null pointer");
    if ((((uintptr_t)labels | (uintptr_t)row_first | (uintptr_t)table) & 3) || (((uintptr_t)fg | (uintptr_t)state) & 7))
        return cvx_fail("pick_emit", "misaligned pointer");
    const BitDims d = bit_dims(D, H, W);
    if (workspace_bytes < bitmap_bytes(d)) return cvx_fail("pick_emit", "workspace shorter than cvx_pick_workspace_bytes");
    const long words = bitmap_words(d);
    CVX_HIP(hipMemsetAsync(table, 0, (size_t)P * CVX_PICK_COLS * sizeof(int32_t), st));  // a P above the state's count leaves zero rows
    hipLaunchKernelGGL(k_pick_place, dim3(blocks_of(words)), dim3(kCclThreads), 0, st, labels, (const Word*)state + words, d, words, row_first, P, table);
    if (const int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_pick_moments, dim3(wave_blocks_of(P)), dim3(kCclThreads), 0, st, (const Word*)fg, d, radius, P, table);
    return cvx_check_launch();
}
