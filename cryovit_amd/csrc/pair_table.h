// The pair table shared by nearest.hip (contacts: instance a, nearest instance b within a radius) and overlap.hip (overlaps:
// instance a and instance b on the same voxel): an open-addressed table in device memory, keyed a << 32 | b, with a count and a
// 64-bit minimum per slot, filled by a claim pass and an accumulate pass (the header of nearest.hip says why every key ends in
// exactly one slot and why the rows depend on neither capacity nor scheduling).  Integer atomics only.  The kernels that
// initialise it and read its rows out, the two device functions the passes call, and the host helper that lays the table out
// over the caller's int64 [3][capacity].  Every includer compiles its own copy; the two kernels are static so that the copies
// do not meet at link time.
#pragma once
#include "entry_checks.h"

namespace cvx {

typedef long long nkey_t;
constexpr nkey_t kPairEmpty = LLONG_MAX;  // no pair key reaches it: a, b <= INT32_MAX

struct PairTable {
    nkey_t* keys;               // [capacity], kPairEmpty or a << 32 | b
    unsigned long long* count;  // [capacity]
    nkey_t* lo;                 // [capacity], gap_d2 << 32 | voxel index
    long long* status;          // [0]: 1 when a key found no slot, [1]: claimed slots = P
    unsigned long mask;         // capacity - 1, capacity a power of two
    int shift;                  // 64 - log2(capacity)
};

__device__ __forceinline__ unsigned long pair_slot(const PairTable& t, nkey_t key) {
    return t.mask ? ((unsigned long)key * 0x9E3779B97F4A7C15ul) >> t.shift : 0;
}

static __global__ __launch_bounds__(kCclThreads) void k_pair_init(PairTable t) {
    const unsigned long i = (unsigned long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i < 2) t.status[i] = 0;
    if (i > t.mask) return;
    t.keys[i] = kPairEmpty;
    t.count[i] = 0;
    t.lo[i] = LLONG_MAX;
}

__device__ __forceinline__ void pair_claim(const PairTable& t, nkey_t key) {
    unsigned long s = pair_slot(t, key);
    for (unsigned long probes = 0; probes <= t.mask; ++probes, s = (s + 1) & t.mask) {
        // slots move one way only: a plain read that already shows the key, or a smaller one, spares the atomic
        const nkey_t seen = *(volatile nkey_t*)(t.keys + s);
        if (seen == key) return;
        if (seen < key) continue;
        const nkey_t old = atomicMin(t.keys + s, key);
        if (old == key) return;
        if (old == kPairEmpty) {
            atomicAdd((unsigned long long*)(t.status + 1), 1ull);
            return;
        }
        if (old > key) key = old;  // displaced: it goes on from the next slot, which is the next of its own path too
    }
    atomicMax(t.status, 1LL);  // every slot seen full: the table is too small
}

__device__ __forceinline__ void pair_accumulate(const PairTable& t, nkey_t key, long long count, nkey_t lo) {
    unsigned long s = pair_slot(t, key);
    for (unsigned long probes = 0; probes <= t.mask; ++probes, s = (s + 1) & t.mask) {
        if (t.keys[s] != key) continue;
        atomicAdd(t.count + s, (unsigned long long)count);
        if (lo < *(volatile nkey_t*)(t.lo + s)) atomicMin(t.lo + s, lo);
        return;
    }  // not found: only in a table that overflowed, which the caller discards
}

static __global__ __launch_bounds__(kCclThreads) void k_pair_rows(PairTable t, const long long* __restrict__ order, long p, long long* __restrict__ rows) {
    const long i = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (i >= p) return;
    const unsigned long s = (unsigned long)order[i];
    long long* r = rows + i * CVX_PAIR_COLS;
    if (s > t.mask || t.keys[s] == kPairEmpty) {  // not a claimed slot: the caller's order is wrong
        r[0] = r[1] = r[3] = r[4] = -1;
        r[2] = 0;
        return;
    }
    const nkey_t key = t.keys[s], lo = t.lo[s];
    r[0] = key >> 32;
    r[1] = (int)(key & 0xffffffffLL);
    r[2] = (long long)t.count[s];
    r[3] = lo >> 32;
    r[4] = lo & 0xffffffffLL;
}

// the table over the caller's buffers; false: capacity is no power of two in 1..CVX_PAIR_MAX_CAPACITY
inline bool pair_table(int64_t* table, long capacity, int64_t* status, PairTable& t) {
    if (capacity < 1 || capacity > CVX_PAIR_MAX_CAPACITY || (capacity & (capacity - 1))) return false;
    int log2c = 0;
    while ((1L << log2c) < capacity) ++log2c;
    t = PairTable{(nkey_t*)table, (unsigned long long*)table + capacity, (nkey_t*)table + 2 * capacity, (long long*)status,
                  (unsigned long)capacity - 1, 64 - log2c};
    return true;
}

}  // namespace cvx
