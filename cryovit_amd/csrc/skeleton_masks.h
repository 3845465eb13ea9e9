// The (26,6) simple-point test of the centreline thinning (skeleton.hip) on a voxel's 27-bit "same id" neighbour mask, bit
// (dz+1)*9 + (dy+1)*3 + (dx+1) as in shape.hip (bit 13 = the voxel itself, ignored here).  Plain C++ so that a host program
// (tools/skeleton_masks.cpp) can print the adjacency masks and run the very predicate the kernel runs; the kernel includes it
// as device code.
//
// v is SIMPLE iff (a) its set neighbours are non-empty and form one 26-connected set, and (b) the unset positions of its
// 18-neighbourhood that are face neighbours of v are non-empty and lie in one set connected through face steps within the unset
// 18-neighbourhood positions.  Both are flood fills on the mask: a position that is reached adds its compile-time adjacency mask,
// the result is cut back to the allowed positions, until nothing is added.
#pragma once
#include <stdint.h>
#include <type_traits>
#include <utility>

#ifdef __HIP__
#define CVX_SK_HD __host__ __device__
#else
#define CVX_SK_HD
#endif

namespace cvx {

constexpr int kSkCentre = 13;

CVX_SK_HD constexpr int sk_abs(int v) { return v < 0 ? -v : v; }
CVX_SK_HD constexpr int sk_dz(int b) { return b / 9 - 1; }
CVX_SK_HD constexpr int sk_dy(int b) { return b / 3 % 3 - 1; }
CVX_SK_HD constexpr int sk_dx(int b) { return b % 3 - 1; }
// how many coordinates of position b are not 0: 0 = the centre, 1 = a face neighbour, 2 = edge, 3 = corner
CVX_SK_HD constexpr int sk_kind(int b) { return sk_abs(sk_dz(b)) + sk_abs(sk_dy(b)) + sk_abs(sk_dx(b)); }

// the positions of the given kinds, one bit of `kinds` per kind
CVX_SK_HD constexpr uint32_t sk_positions(int kinds) {
    uint32_t m = 0;
    for (int b = 0; b < 27; ++b)
        if (kinds >> sk_kind(b) & 1) m |= 1u << b;
    return m;
}
constexpr uint32_t kSkN26 = sk_positions(2 | 4 | 8), kSkN18 = sk_positions(2 | 4), kSkN6 = sk_positions(2);

// the positions (centre aside) that touch position b by a face, an edge or a corner
CVX_SK_HD constexpr uint32_t sk_adj26(int b) {
    uint32_t m = 0;
    for (int c = 0; c < 27; ++c) {
        const int az = sk_abs(sk_dz(b) - sk_dz(c)), ay = sk_abs(sk_dy(b) - sk_dy(c)), ax = sk_abs(sk_dx(b) - sk_dx(c));
        if (c != b && c != kSkCentre && az <= 1 && ay <= 1 && ax <= 1) m |= 1u << c;
    }
    return m;
}

// the positions of the 18-neighbourhood one face step from position b
CVX_SK_HD constexpr uint32_t sk_adj6(int b) {
    uint32_t m = 0;
    for (int c = 0; c < 27; ++c)
        if ((kSkN18 >> c & 1) && sk_abs(sk_dz(b) - sk_dz(c)) + sk_abs(sk_dy(b) - sk_dy(c)) + sk_abs(sk_dx(b) - sk_dx(c)) == 1) m |= 1u << c;
    return m;
}

// the adjacency masks of the positions of `seen`, as compile-time constants
template <bool FACE, int... B>
CVX_SK_HD inline uint32_t sk_grow(uint32_t seen, std::integer_sequence<int, B...>) {
    return (seen | ... | ((0u - (seen >> B & 1u)) & std::integral_constant<uint32_t, FACE ? sk_adj6(B) : sk_adj26(B)>::value));
}

// the positions of `within` reachable from `seed` (a subset of it): face steps (FACE) or 26-adjacency
template <bool FACE>
CVX_SK_HD inline uint32_t sk_flood(uint32_t seed, uint32_t within) {
    uint32_t seen = seed;
    for (;;) {
        const uint32_t grow = sk_grow<FACE>(seen, std::make_integer_sequence<int, 27>{}) & within;
        if (grow == seen) return seen;
        seen = grow;
    }
}

CVX_SK_HD inline bool sk_simple(uint32_t m) {
    m &= kSkN26;
    if (m == 0) return false;
    if (sk_flood<false>(m & (0u - m), m) != m) return false;
    const uint32_t unset = ~m & kSkN18, faces = unset & kSkN6;
    if (faces == 0) return false;
    return (faces & ~sk_flood<true>(faces & (0u - faces), unset)) == 0;
}

}  // namespace cvx
