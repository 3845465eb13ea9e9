// What the distance map (edt.hip) and the nearest-instance map (nearest.hip) share: the site bitmaps of the row pass, the
// pruned min-plus walk of the line passes and its tiling, and the geometry of the lines.
#pragma once
#include "common.h"
#include "../../include/cryovit_hip.h"

#include <limits.h>

namespace cvx {

constexpr int kEdtNone = CVX_EDT_NONE;
constexpr int kRowThreads = 256;           // x pass: 4 waves = 4 rows per workgroup
constexpr int kSlab = 64;                  // min-plus passes: adjacent x per workgroup = lanes of a wave
constexpr int kIpt = 8;                    // outputs per thread
constexpr int kJu = 8;                     // sources fetched per pruning test
constexpr int kLineWavesMax = 16;

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// ---- x pass: the sites of a row as 64-voxel bitmaps ----

// One wave per row.  Leaves in LDS the row's nc site bitmaps (the wave's ballots of site(x)) and per bitmap the last site of all
// earlier bitmaps (-1: none) and the first site of all later ones (INT_MAX: none): a forward max-scan over the bitmaps' last
// sites and a backward min-scan over their first sites, one lane per bitmap, 64 bitmaps per round of shuffles.  Every wave of the
// workgroup calls it (two barriers); afterwards edt_row_sides finds a voxel's nearest site on either side without a walk.
struct RowSites {
    const unsigned long long* bits;
    const int* before;
    const int* after;
};

template <class Site>
__device__ __forceinline__ RowSites edt_row_sites(unsigned long long* lds, int nc, Site site) {
    const int lane = threadIdx.x & 63;
    unsigned long long* bits = lds + (long)wave_id() * 2 * nc;  // per wave: nc bitmaps, then nc ints twice
    int* before = (int*)(bits + nc);
    int* after = before + nc;
    for (int c = 0; c < nc; ++c) {
        const unsigned long long b = __ballot(site(c * 64 + lane));
        if (lane == 0) bits[c] = b;
    }
    __syncthreads();
    int carry = -1;  // forward: the last site of all earlier bitmaps
    for (int base = 0; base < nc; base += 64) {
        const int c = base + lane;
        const unsigned long long b = c < nc ? bits[c] : 0;
        int v = b ? c * 64 + 63 - __clzll((long long)b) : -1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(v, o, 64);
            if (lane >= o) v = max(v, t);
        }
        int excl = __shfl_up(v, 1, 64);
        if (lane == 0) excl = -1;
        if (c < nc) before[c] = max(excl, carry);
        carry = max(carry, __shfl(v, 63, 64));
    }
    carry = INT_MAX;  // backward: the first site of all later bitmaps
    for (int base = (nc - 1) / 64 * 64; base >= 0; base -= 64) {
        const int c = base + lane;
        const unsigned long long b = c < nc ? bits[c] : 0;
        int v = b ? c * 64 + __ffsll((unsigned long long)b) - 1 : INT_MAX;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_down(v, o, 64);
            if (lane + o < 64) v = min(v, t);
        }
        int excl = __shfl_down(v, 1, 64);
        if (lane == 63) excl = INT_MAX;
        if (c < nc) after[c] = min(excl, carry);
        carry = min(carry, __shfl(v, 0, 64));
    }
    __syncthreads();
    return RowSites{bits, before, after};
}

// the nearest site at or before x = c * 64 + lane (-1: none) and at or after it (INT_MAX: none)
__device__ __forceinline__ void edt_row_sides(const RowSites& r, int c, int lane, int& left, int& right) {
    const unsigned long long b = r.bits[c];
    const unsigned long long lo = b & (~0ull >> (63 - lane)), hi = b >> lane;
    left = lo ? c * 64 + 63 - __clzll((long long)lo) : r.before[c];
    right = hi ? c * 64 + lane + __ffsll(hi) - 1 : r.after[c];
}

inline size_t edt_row_lds_bytes(int nc) { return (size_t)(kRowThreads / 64) * nc * 16; }  // <= 46 KB: W <= 46341

// ---- y and z passes: the min-plus walk ----

// best[k] = min(best[k], f(j) + (i0 + k - j)^2) for the sources j of [ja, jb), walked downwards from the thread's last output
// and upwards from the source after it, kJu sources per pruning test.  MODE 0: every pair; 1: pairs with j <= i only; 2: pairs
// with j >= i only.  i0 is the same for the whole wave; lanes that are not `active` (past the row's end) hold no minimum and do
// not keep the walk going.  V says what a value is: V::T; V::none() and V::is_none(v); V::step(v, dd) = v moved by the squared
// step dd; V::d2(v) = its squared distance; V::kTies: whether a value at the SAME distance can still be smaller (a key that
// carries an id), in which case the walk may only stop once the squared step alone EXCEEDS the widest distance the wave holds,
// where reaching it is enough for a plain distance.
struct EdtDistance {
    typedef int T;
    static constexpr bool kTies = false;
    __device__ static T none() { return kEdtNone; }
    __device__ static bool is_none(T v) { return v == kEdtNone; }
    __device__ static T step(T v, int dd) { return v + dd; }
    __device__ static int d2(T v) { return v; }
};

template <class V, int MODE, class F>
__device__ __forceinline__ void edt_minplus(F f, bool active, int i0, int ja, int jb, typename V::T (&best)[kIpt]) {
    typedef typename V::T T;
    auto take = [&](int j, T v) {
        if (V::is_none(v)) return;
#pragma unroll
        for (int k = 0; k < kIpt; ++k) {
            const int d = i0 + k - j;
            if ((MODE == 1 && d < 0) || (MODE == 2 && d > 0)) continue;
            best[k] = min(best[k], V::step(v, d * d));
        }
    };
    auto widest = [&]() {
        T m = best[0];
#pragma unroll
        for (int k = 1; k < kIpt; ++k) m = max(m, best[k]);
        return V::d2(m);
    };
    auto live = [&](int gap) { return V::kTies ? gap * gap <= widest() : gap * gap < widest(); };
    const int top = min(i0 + kIpt, jb);  // sources below top go to the downward walk
    if (MODE != 2 || top > i0) {
        const int stop = MODE == 2 ? max(ja, i0) : ja;
        for (int j1 = top; j1 > stop; j1 -= kJu) {
            const int gap = i0 - (j1 - 1);  // the step from the nearest source of this group to the nearest output
            if (gap > 0 && !__any(active && live(gap))) break;
            T v[kJu];
#pragma unroll
            for (int u = 0; u < kJu; ++u) v[u] = j1 - 1 - u >= stop ? f(j1 - 1 - u) : V::none();
#pragma unroll
            for (int u = 0; u < kJu; ++u) take(j1 - 1 - u, v[u]);
        }
    }
    if (MODE != 1) {
        for (int j0 = max(top, ja); j0 < jb; j0 += kJu) {
            const int gap = j0 - (i0 + kIpt - 1);
            if (gap > 0 && !__any(active && live(gap))) break;
            T v[kJu];
#pragma unroll
            for (int u = 0; u < kJu; ++u) v[u] = j0 + u < jb ? f(j0 + u) : V::none();
#pragma unroll
            for (int u = 0; u < kJu; ++u) take(j0 + u, v[u]);
        }
    }
}

struct LineGeom {
    int n;         // elements of a line
    long stride;   // between two of them
    long ostride;  // between two lines of one slab column
    int W, nslab;  // row length, slabs per row
};

}  // namespace cvx
