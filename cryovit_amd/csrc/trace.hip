// Filament tracing (`--trace`): the skeleton graph of every instance as branches (chains of path voxels between node voxels, closed
// rings, links), each voxel with its branch, its rank along it and the step counts up to it.  The definition (neighbour, path and
// node voxel, chain, ring, link, key voxel, both tables) is in include/cryovit_hip.h.  Integers only, no float atomics; the only
// atomics are the integer sum / min / max of d2 into a branch row, whose result does not depend on their order.  No kernel reads a
// word that the same launch writes.
//
// COUNT.  k_trace_classify, one wave per 64 voxels of a row: the id of the lane's voxel (outside 1..k = 0), its 26 same-id
//   neighbours straight from the volume (a skeleton is a few voxels per thousand, so only those lanes read a neighbourhood and an
//   LDS tile would be loaded for nothing), two __ballots: "a voxel" and "a path voxel" as bits (bit_rows.h).  k_trace_count: both
//   counts per row; k_trace_scan: one workgroup, exclusive prefix sums in row order and the total (k_pick_scan's form).
// EMIT.  k_trace_emit, one wave per word: a voxel's slot = its row's first slot + popcount(the bits before it); z, y, x, id, degree
//   and d2 go to the voxel table, the slots of the (at most two) neighbours of an end or path voxel to nbrs[slot][2], the
//   neighbour with the smaller index first.  The other columns are cleared.
// RANK.  Pointer doubling over direction states: state 2 v + j = "at path voxel v, travelling towards nbrs[v][j]".  Its successor is
//   the state of that neighbour that does not point back; where the neighbour is a node voxel (or the cut voxel of v's ring) the
//   state is a fixed point.  A state carries its pointer, the (f, e, c) steps from v to the pointer's voxel and the smallest slot
//   seen on the way.  k_trace_init writes the states, k_trace_round composes every state with the one it points to, from one
//   buffer into the other: in place a state could read a pointer that this round already advanced and skip voxels.  After
//   ceil(log2 Np) rounds every chain state points to the fixed point at its end of the chain.  A state whose pointer is no fixed
//   point (or points to itself over 2^rounds steps: a ring of 4, 8, ... voxels) lies on a ring and has seen the whole ring:
//   k_trace_rings marks those voxels with the ring's smallest slot m, and the
//   same rounds run once more with m as a cut, after which a ring state ends at the voxel before m in its direction.
// FINALISE.  k_trace_ranks, one thread per voxel: from its two end states the head, the direction that leads back to the start,
//   rank and step counts; key flags (head of a chain, m of a ring, key end of a link).  k_trace_scan numbers the keys.
//   k_trace_rows: every path voxel gets its branch number, every key voxel writes its branch row by plain stores.
//   k_trace_d2: sum, min and max of d2 over the path voxels of a branch, combined over a wave that holds one branch first.
#include "bit_rows.h"

namespace cvx {

constexpr int kTraceScanThreads = 1024, kTraceScanPer = 4;
constexpr int kVC = CVX_TRACE_VOXEL_COLS, kBC = CVX_TRACE_BRANCH_COLS;
constexpr int kTraceMaxRounds = 32;  // 2^32 > twice any voxel count

struct TraceState {
    unsigned next;     // the state this one has reached; itself at a fixed point
    unsigned f, e, c;  // face, edge and corner steps from the state's own voxel to the voxel of `next` (unsigned: a ring state wraps in the first pass)
    int low;           // the smallest slot among the voxels from its own to that of `next`
};
static_assert(sizeof(TraceState) == CVX_TRACE_STATE_BYTES, "the header states the size of a state");

__device__ __forceinline__ int trace_id(const int* __restrict__ sk, const BitDims& d, int k, int z, int y, int x) {
    if ((unsigned)z >= (unsigned)d.D || (unsigned)y >= (unsigned)d.H || (unsigned)x >= (unsigned)d.W) return 0;
    const int l = sk[((long)z * d.H + y) * d.W + x];
    return l >= 1 && l <= k ? l : 0;
}

// bit b = the b-th of the 26 neighbours in raster order carries `id`
__device__ __forceinline__ unsigned trace_mask(const int* __restrict__ sk, const BitDims& d, int k, int z, int y, int x, int id) {
    unsigned m = 0;
    int bit = 0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (!(dz | dy | dx)) continue;
                if (trace_id(sk, d, k, z + dz, y + dy, x + dx) == id) m |= 1u << bit;
                ++bit;
            }
    return m;
}

// the slot of voxel (z, y, x), a set bit of occ
__device__ __forceinline__ long trace_slot(const Word* __restrict__ occ, const int* __restrict__ row_first, const BitDims& d, int z, int y, int x) {
    const long row = (long)z * d.H + y;
    const Word* p = occ + row * d.WW;
    long slot = row_first[row];
    for (int u = 0; u < x >> 6; ++u) slot += __popcll(p[u]);
    return slot + __popcll(p[x >> 6] & ((1ull << (x & 63)) - 1));
}

// the step between two rows of the voxel table as 1 face, 2 edge, 3 corner; 0 when they are no neighbours
__device__ __forceinline__ int trace_step(const int* a, const int* b) {
    const int dz = abs(a[0] - b[0]), dy = abs(a[1] - b[1]), dx = abs(a[2] - b[2]);
    return max(dz, max(dy, dx)) == 1 ? dz + dy + dx : 0;
}
__device__ __forceinline__ void trace_add_step(int cls, unsigned& f, unsigned& e, unsigned& c) {
    f += cls == 1, e += cls == 2, c += cls == 3;
}

// ---- count ----

__global__ __launch_bounds__(kCclThreads) void k_trace_classify(const int* __restrict__ sk, BitDims d, long words, int k, Word* __restrict__ bits) {
    long g, row;
    int x;
    if (!wave_word(d.WW, words, g, row, x)) return;
    const int y = (int)(row % d.H), z = (int)(row / d.H);
    int id = 0;
    if (x < d.W) {
        id = sk[row * d.W + x];
        id = id >= 1 && id <= k ? id : 0;
    }
    const bool path = id && __popc(trace_mask(sk, d, k, z, y, x, id)) == 2;
    const Word occ = __ballot(id != 0), pth = __ballot(path);
    if ((threadIdx.x & 63) == 0) {
        bits[g] = occ;
        bits[words + g] = pth;
    }
}

// counts[r] = the voxels of row r, counts[rows + r] = its path voxels
__global__ __launch_bounds__(kCclThreads) void k_trace_count(const Word* __restrict__ bits, long rows, int WW, int* __restrict__ counts) {
    const long r = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (r >= rows) return;
    const long words = rows * WW;
    int n = 0, np = 0;
    for (int w = 0; w < WW; ++w) {
        n += __popcll(bits[r * WW + w]);
        np += __popcll(bits[words + r * WW + w]);
    }
    counts[r] = n;
    counts[rows + r] = np;
}

// a[i] = the sum of a[0..i), in place; total = the sum (below 2^31: it counts voxels)
__global__ __launch_bounds__(kTraceScanThreads) void k_trace_scan(int* __restrict__ a, long n, long long* __restrict__ total) {
    constexpr int kWaves = kTraceScanThreads / 64;
    __shared__ int wsum[kWaves];
    const int wave = threadIdx.x >> 6;
    long long carry = 0;
    for (long base = 0; base < n; base += kTraceScanThreads * kTraceScanPer) {
        const long i0 = base + (long)threadIdx.x * kTraceScanPer;
        int v[kTraceScanPer], sv = 0;
#pragma unroll
        for (int j = 0; j < kTraceScanPer; ++j) {
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
        for (int j = 0; j < kTraceScanPer; ++j)
            if (i0 + j < n) {
                a[i0 + j] = (int)run;
                run += v[j];
            }
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// ---- emit ----

__global__ __launch_bounds__(kCclThreads) void k_trace_emit(const int* __restrict__ sk, const int* __restrict__ d2, const Word* __restrict__ occ,
                                                            const int* __restrict__ row_first, BitDims d, long words, int k, long N,
                                                            int* __restrict__ voxels, int* __restrict__ nbrs) {
    long g, row;
    int x;
    if (!wave_word(d.WW, words, g, row, x)) return;
    const int lane = threadIdx.x & 63, w = (int)(g % d.WW);
    Word own = occ[g];
    if (w == d.WW - 1) own &= tail_mask(d.W);  // a bit past W is no voxel, whatever the bitmap holds
    if (!(own >> lane & 1)) return;
    const int y = (int)(row % d.H), z = (int)(row / d.H);
    const long slot = trace_slot(occ, row_first, d, z, y, x);
    if (slot >= N) return;  // an N that is not this bitmap's count: write nothing past the tables
    const int id = trace_id(sk, d, k, z, y, x);
    const unsigned m = id ? trace_mask(sk, d, k, z, y, x, id) : 0;
    const int deg = __popc(m);
    int dist = d2 ? d2[row * d.W + x] : 0;
    if (dist == CVX_EDT_NONE) dist = 0;
    int* t = voxels + slot * kVC;
    t[0] = z, t[1] = y, t[2] = x, t[3] = id, t[4] = deg;
    t[5] = t[6] = t[7] = t[8] = t[9] = 0;
    t[10] = dist, t[11] = 0;
    long nb[2] = {-1, -1};
    if (deg <= 2) {
        unsigned rest = m;
        for (int j = 0; j < deg; ++j) {
            const int b = __ffs((int)rest) - 1;
            rest &= rest - 1;
            const int cell = b < 13 ? b : b + 1;  // the centre is no neighbour
            const int nz = z + cell / 9 - 1, ny = y + cell / 3 % 3 - 1, nx = x + cell % 3 - 1;
            const long s = trace_slot(occ, row_first, d, nz, ny, nx);
            nb[j] = s < N ? s : -1;
        }
    }
    nbrs[2 * slot] = (int)nb[0];
    nbrs[2 * slot + 1] = (int)nb[1];
}

// ---- rank ----

__device__ __forceinline__ bool trace_is_path(const int* __restrict__ voxels, long v, long N) { return (unsigned long)v < (unsigned long)N && voxels[v * kVC + 4] == 2; }

__global__ __launch_bounds__(kCclThreads) void k_trace_init(const int* __restrict__ voxels, const int* __restrict__ nbrs, const int* __restrict__ cut,
                                                            long N, TraceState* __restrict__ out) {
    const long s = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (s >= 2 * N) return;
    const long v = s >> 1;
    TraceState o{(unsigned)s, 0u, 0u, 0u, (int)v};
    if (trace_is_path(voxels, v, N)) {
        const long w = nbrs[s];
        if (trace_is_path(voxels, w, N) && !(cut && cut[v] == w)) {
            o.next = (unsigned)(2 * w + (nbrs[2 * w] == v ? 1 : 0));  // the direction of w that does not point back
            trace_add_step(trace_step(voxels + v * kVC, voxels + w * kVC), o.f, o.e, o.c);
            o.low = (int)min(v, w);
        }
    }
    out[s] = o;
}

__global__ __launch_bounds__(kCclThreads) void k_trace_round(const TraceState* __restrict__ in, long N, TraceState* __restrict__ out) {
    const long s = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (s >= 2 * N) return;
    TraceState a = in[s];
    if (a.next < 2 * (unsigned long)N) {
        const TraceState b = in[a.next];  // a fixed point adds nothing
        a.next = b.next;
        a.f += b.f, a.e += b.e, a.c += b.c;
        a.low = min(a.low, b.low);
    }
    out[s] = a;
}

// cut[v] = the smallest slot of v's ring, -1 off a ring; *any = 1 when there is a ring (a plain store: every writer stores 1)
__global__ __launch_bounds__(kCclThreads) void k_trace_rings(const int* __restrict__ voxels, const TraceState* __restrict__ st, long N,
                                                             int* __restrict__ cut, int* __restrict__ any) {
    const long v = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (v >= N) return;
    int m = -1;
    if (voxels[v * kVC + 4] == 2) {
        const TraceState a = st[2 * v];
        if (a.next < 2 * (unsigned long)N) {
            // a chain state has reached a fixed point: a state that points to itself over no step.  On a ring whose length divides
            // the 2^rounds steps taken, a state points to itself too, but over that many steps
            const TraceState b = st[a.next];
            if (b.next != a.next || (b.f | b.e | b.c)) {
                m = a.low;
                *any = 1;
            }
        }
    }
    cut[v] = m;
}

// ---- finalise ----

// of path voxel v: the key voxel of its branch, the direction `back` of v that leads to the branch's start, whether it is a ring
struct TraceSide {
    long head;
    int back;
    bool ring;
};

__device__ __forceinline__ TraceSide trace_side(const int* __restrict__ nbrs, const TraceState* __restrict__ st, const int* __restrict__ cut, long v) {
    const long m = cut ? cut[v] : -1;
    const long xa = st[2 * v].next >> 1, xb = st[2 * v + 1].next >> 1;  // where the two directions end
    if (m >= 0) return TraceSide{m, v == m ? 1 : xa == nbrs[2 * m] ? 0 : 1, true};  // backwards a ring ends at m's first neighbour
    if (xa == xb) return TraceSide{v, 0, false};  // a chain of one voxel starts at its smaller neighbour
    const long head = min(xa, xb);
    return TraceSide{head, xa == head ? 0 : 1, false};
}

// an end voxel v is the key of a link when its only neighbour w is a node voxel, and of two ends the smaller
__device__ __forceinline__ bool trace_link_key(const int* __restrict__ voxels, const int* __restrict__ nbrs, long N, long v) {
    const long w = nbrs[2 * v];
    if ((unsigned long)w >= (unsigned long)N) return false;
    const int dw = voxels[w * kVC + 4];
    return dw != 2 && !(dw == 1 && w < v);
}

__device__ __forceinline__ bool trace_in(long v, long N) { return (unsigned long)v < (unsigned long)N; }

// rank, step counts and ring flag of every path voxel (its own row's columns 6 .. 9 and 11); keys[v] = 1 on a key voxel
__global__ __launch_bounds__(kCclThreads) void k_trace_ranks(int* __restrict__ voxels, const int* __restrict__ nbrs, const TraceState* __restrict__ st,
                                                             const int* __restrict__ cut, long N, int* __restrict__ keys) {
    const long v = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (v >= N) return;
    int* t = voxels + v * kVC;
    const int deg = t[4];
    int key = 0;
    if (deg == 1) key = trace_link_key(voxels, nbrs, N, v);
    if (deg == 2 && st) {
        const TraceSide side = trace_side(nbrs, st, cut, v);
        const TraceState bk = st[2 * v + side.back];
        unsigned f = bk.f, e = bk.e, c = bk.c;
        int rank = 1;
        if (side.ring) {
            if (v == side.head) {
                f = e = c = 0;
            } else {
                const long first = nbrs[2 * side.head];  // rank 2
                if (trace_in(first, N)) trace_add_step(trace_step(voxels + side.head * kVC, voxels + first * kVC), f, e, c);
                rank = (int)(bk.f + bk.e + bk.c) + 2;
            }
        } else {
            const long h = bk.next >> 1;
            const long start = trace_in(h, N) ? nbrs[bk.next] : -1;
            if (trace_in(start, N)) trace_add_step(trace_step(voxels + start * kVC, voxels + h * kVC), f, e, c);
            rank = (int)(bk.f + bk.e + bk.c) + 1;
        }
        t[6] = rank, t[7] = (int)f, t[8] = (int)e, t[9] = (int)c, t[11] = side.ring;
        key = v == side.head;
    }
    keys[v] = key;
}

__device__ __forceinline__ long long trace_index(const int* t, int H, int W) { return ((long long)t[0] * H + t[1]) * W + t[2]; }

// first = the scanned keys.  The branch number of every path voxel (column 5 of its own row) and the branch rows of the key voxels
__global__ __launch_bounds__(kCclThreads) void k_trace_rows(int* __restrict__ voxels, const int* __restrict__ nbrs, const TraceState* __restrict__ st,
                                                            const int* __restrict__ cut, const int* __restrict__ first, int H, int W, long N, long B,
                                                            long long* __restrict__ branches) {
    const long v = (long)blockIdx.x * kCclThreads + threadIdx.x;
    if (v >= N) return;
    int* t = voxels + v * kVC;
    const int deg = t[4];
    long start = -1, end = -1, head = -1, last = -1, n = 0;
    unsigned f = 0, e = 0, c = 0;
    bool ring = false;
    if (deg == 1) {
        if (!trace_link_key(voxels, nbrs, N, v)) return;
        start = v, end = nbrs[2 * v];
        trace_add_step(trace_step(t, voxels + end * kVC), f, e, c);
    } else if (deg == 2 && st) {
        const TraceSide side = trace_side(nbrs, st, cut, v);
        if (!trace_in(side.head, N)) return;
        t[5] = first[side.head] + 1;
        if (v != side.head) return;
        const TraceState fw = st[2 * v + 1 - side.back];  // from the head to the last path voxel
        head = v, last = fw.next >> 1, n = (long)(fw.f + fw.e + fw.c) + 1, ring = side.ring;
        if (!trace_in(last, N)) return;
        start = ring ? v : nbrs[2 * v + side.back];
        end = ring ? v : nbrs[fw.next];
        if (!trace_in(start, N) || !trace_in(end, N)) return;
        f = fw.f, e = fw.e, c = fw.c;
        trace_add_step(trace_step(voxels + last * kVC, voxels + end * kVC), f, e, c);
        if (!ring) trace_add_step(trace_step(voxels + start * kVC, t), f, e, c);
    } else {
        return;
    }
    const long r = first[v];
    if (r >= B) return;  // a B that is not this table's count: write nothing past the rows
    const int* ts = voxels + start * kVC;
    const int* te = voxels + end * kVC;
    const int ds = ts[4], de = te[4];
    const long long oz = ts[0] - te[0], oy = ts[1] - te[1], ox = ts[2] - te[2];
    long long* row = branches + r * kBC;
    row[0] = t[3];
    row[1] = ring ? 3 : (ds >= 3) + (de >= 3);
    row[2] = n;
    row[3] = f, row[4] = e, row[5] = c;
    row[6] = trace_index(ts, H, W), row[7] = trace_index(te, H, W);
    row[8] = ds, row[9] = de;
    row[10] = 0;
    row[11] = n ? LLONG_MAX : 0;  // k_trace_d2 brings every path voxel's d2 in
    row[12] = n ? LLONG_MIN : 0;
    row[13] = head >= 0 ? trace_index(voxels + head * kVC, H, W) : -1;
    row[14] = last >= 0 ? trace_index(voxels + last * kVC, H, W) : -1;
    row[15] = oz * oz + oy * oy + ox * ox;
}

__global__ __launch_bounds__(kCclThreads) void k_trace_d2(const int* __restrict__ voxels, long N, long B, long long* __restrict__ branches) {
    const long v = (long)blockIdx.x * kCclThreads + threadIdx.x;
    int cur = 0, dist = 0;
    if (v < N) {
        const int* t = voxels + v * kVC;
        if (t[4] == 2 && t[5] >= 1 && t[5] <= B) cur = t[5], dist = t[10];
    }
    const int one = wave_single_id(cur);
    long long sum = dist, lo = dist, hi = dist;
    if (one) {
        sum = wave_sum((long long)(cur ? dist : 0));
        lo = wave_min(cur ? dist : INT_MAX);
        hi = wave_max(cur ? dist : INT_MIN);
        const unsigned long long has = __ballot(cur != 0);
        if ((threadIdx.x & 63) != __ffsll((long long)has) - 1) cur = 0;  // the first lane of the branch speaks for the wave
    }
    if (!cur) return;
    long long* row = branches + (long)(cur - 1) * kBC;
    if (sum) atomicAdd((unsigned long long*)row + 10, (unsigned long long)sum);
    table_min(row + 11, lo);
    table_max(row + 12, hi);
}

}  // namespace cvx

using namespace cvx;

namespace {

// what every entry refuses about the volume.  nullptr: fine
const char* trace_fault(int D, int H, int W, long k, long& n) {
    if (const char* why = extents_fault(D, H, W, kExtentMax, n)) return why;
    if (k < 0) return "k < 0";
    return nullptr;
}

bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

}  // namespace

extern "C" long cvx_trace_workspace_bytes(int D, int H, int W) { return bitmap_workspace_bytes(D, H, W); }

extern "C" int cvx_trace_count(const int32_t* sk, int D, int H, int W, long k, uint64_t* bits, long workspace_bytes, int32_t* row_first,
                               int64_t* totals, hipStream_t st) {
    long n = 0;
    if (const char* why = trace_fault(D, H, W, k, n)) return cvx_fail("trace_count", why);
    if (!totals) return cvx_fail("trace_count", "null pointer");
    if (misaligned(totals, 7)) return cvx_fail("trace_count", "misaligned pointer");
    if (n > 0 && k > 0) {
        if (!sk || !bits || !row_first) return cvx_fail("trace_count", "null pointer");
        if (misaligned(sk, 3) || misaligned(row_first, 3) || misaligned(bits, 7)) return cvx_fail("trace_count", "misaligned pointer");
        if (workspace_bytes < bitmap_bytes(bit_dims(D, H, W))) return cvx_fail("trace_count", "workspace shorter than cvx_trace_workspace_bytes");
    }
    CVX_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), st));
    if (n == 0 || k == 0) return 0;
    const BitDims d = bit_dims(D, H, W);
    const long rows = (long)D * H, words = bitmap_words(d);
    hipLaunchKernelGGL(k_trace_classify, dim3(wave_blocks_of(words)), dim3(kCclThreads), 0, st, sk, d, words, clamp_int(k), (Word*)bits);
    if (const int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_trace_count, dim3(blocks_of(rows)), dim3(kCclThreads), 0, st, (const Word*)bits, rows, d.WW, row_first);
    if (const int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_trace_scan, dim3(1), dim3(kTraceScanThreads), 0, st, row_first, rows, (long long*)totals);
    if (const int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_trace_scan, dim3(1), dim3(kTraceScanThreads), 0, st, row_first + rows, rows, (long long*)totals + 1);
    return cvx_check_launch();
}

extern "C" int cvx_trace_emit(const int32_t* sk, const int32_t* d2, const uint64_t* bits, const int32_t* row_first, int D, int H, int W, long k,
                              long workspace_bytes, long N, int32_t* voxels, int32_t* nbrs, hipStream_t st) {
    long n = 0;
    if (const char* why = trace_fault(D, H, W, k, n)) return cvx_fail("trace_emit", why);
    if (N < 0 || N > n) return cvx_fail("trace_emit", "N outside [0, D*H*W]");
    if (N == 0 || k == 0) return 0;
    if (!sk || !bits || !row_first || !voxels || !nbrs) return cvx_fail("trace_emit", "null pointer");
    if (misaligned(sk, 3) || misaligned(d2, 3) || misaligned(row_first, 3) || misaligned(voxels, 3) || misaligned(nbrs, 3) || misaligned(bits, 7))
        return cvx_fail("trace_emit", "misaligned pointer");
    const BitDims d = bit_dims(D, H, W);
    if (workspace_bytes < bitmap_bytes(d)) return cvx_fail("trace_emit", "workspace shorter than cvx_trace_workspace_bytes");
    const long words = bitmap_words(d);
    CVX_HIP(hipMemsetAsync(voxels, 0, (size_t)N * kVC * sizeof(int32_t), st));  // an N above the bitmap's count leaves zero rows,
    CVX_HIP(hipMemsetAsync(nbrs, 0xff, (size_t)N * 2 * sizeof(int32_t), st));    // without neighbours
    hipLaunchKernelGGL(k_trace_emit, dim3(wave_blocks_of(words)), dim3(kCclThreads), 0, st, sk, d2, (const Word*)bits, row_first, d, words,
                       clamp_int(k), N, voxels, nbrs);
    return cvx_check_launch();
}

extern "C" int cvx_trace_rank(const int32_t* voxels, const int32_t* nbrs, const int32_t* cut, long N, int rounds, void* state_a, void* state_b,
                              hipStream_t st) {
    if (N < 0 || N > CVX_COMPONENT_MAX_VOXELS) return cvx_fail("trace_rank", "N outside [0, 2^31 - 2]");
    if (rounds < 0 || rounds > kTraceMaxRounds) return cvx_fail("trace_rank", "rounds outside [0, 32]");
    if (N == 0) return 0;
    if (!voxels || !nbrs || !state_a || !state_b) return cvx_fail("trace_rank", "null pointer");
    if (misaligned(voxels, 3) || misaligned(nbrs, 3) || misaligned(cut, 3) || misaligned(state_a, 3) || misaligned(state_b, 3))
        return cvx_fail("trace_rank", "misaligned pointer");
    const uintptr_t a = (uintptr_t)state_a, b = (uintptr_t)state_b, bytes = (uintptr_t)N * 2 * sizeof(TraceState);
    if (a < b + bytes && b < a + bytes) return cvx_fail("trace_rank", "state_a and state_b must not overlap");
    TraceState* buf[2] = {(TraceState*)state_a, (TraceState*)state_b};
    hipLaunchKernelGGL(k_trace_init, dim3(blocks_of(2 * N)), dim3(kCclThreads), 0, st, voxels, nbrs, cut, N, buf[0]);
    if (const int rc = cvx_check_launch()) return rc;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_trace_round, dim3(blocks_of(2 * N)), dim3(kCclThreads), 0, st, (const TraceState*)buf[r % 2], N, buf[1 - r % 2]);
        if (const int rc = cvx_check_launch()) return rc;
    }
    return 0;
}

extern "C" int cvx_trace_rings(const int32_t* voxels, const void* state, long N, int32_t* cut, int32_t* any, hipStream_t st) {
    if (N < 0 || N > CVX_COMPONENT_MAX_VOXELS) return cvx_fail("trace_rings", "N outside [0, 2^31 - 2]");
    if (!any) return cvx_fail("trace_rings", "null pointer");
    if (misaligned(any, 3)) return cvx_fail("trace_rings", "misaligned pointer");
    if (N > 0) {
        if (!voxels || !state || !cut) return cvx_fail("trace_rings", "null pointer");
        if (misaligned(voxels, 3) || misaligned(state, 3) || misaligned(cut, 3)) return cvx_fail("trace_rings", "misaligned pointer");
    }
    CVX_HIP(hipMemsetAsync(any, 0, sizeof(int32_t), st));
    if (N == 0) return 0;
    hipLaunchKernelGGL(k_trace_rings, dim3(blocks_of(N)), dim3(kCclThreads), 0, st, voxels, (const TraceState*)state, N, cut, any);
    return cvx_check_launch();
}

extern "C" int cvx_trace_keys(int32_t* voxels, const int32_t* nbrs, const void* state, const int32_t* cut, long N, int32_t* keys, int64_t* total,
                              hipStream_t st) {
    if (N < 0 || N > CVX_COMPONENT_MAX_VOXELS) return cvx_fail("trace_keys", "N outside [0, 2^31 - 2]");
    if (!total) return cvx_fail("trace_keys", "null pointer");
    if (misaligned(total, 7)) return cvx_fail("trace_keys", "misaligned pointer");
    if (N > 0) {
        if (!voxels || !nbrs || !keys) return cvx_fail("trace_keys", "null pointer");
        if (cut && !state) return cvx_fail("trace_keys", "a cut without a state");
        if (misaligned(voxels, 3) || misaligned(nbrs, 3) || misaligned(state, 3) || misaligned(cut, 3) || misaligned(keys, 3))
            return cvx_fail("trace_keys", "misaligned pointer");
    }
    CVX_HIP(hipMemsetAsync(total, 0, sizeof(int64_t), st));
    if (N == 0) return 0;
    hipLaunchKernelGGL(k_trace_ranks, dim3(blocks_of(N)), dim3(kCclThreads), 0, st, voxels, nbrs, (const TraceState*)state, cut, N, keys);
    if (const int rc = cvx_check_launch()) return rc;
    hipLaunchKernelGGL(k_trace_scan, dim3(1), dim3(kTraceScanThreads), 0, st, keys, N, (long long*)total);
    return cvx_check_launch();
}

extern "C" int cvx_trace_branches(int32_t* voxels, const int32_t* nbrs, const void* state, const int32_t* cut, const int32_t* first, int D, int H,
                                  int W, long N, long B, int64_t* branches, hipStream_t st) {
    long n = 0;
    if (const char* why = trace_fault(D, H, W, 0, n)) return cvx_fail("trace_branches", why);
    if (N < 0 || N > n) return cvx_fail("trace_branches", "N outside [0, D*H*W]");
    if (B < 0 || B > N) return cvx_fail("trace_branches", "B outside [0, N]");
    if (N == 0) return 0;
    if (!voxels || !nbrs || !first || (B > 0 && !branches)) return cvx_fail("trace_branches", "null pointer");
    if (cut && !state) return cvx_fail("trace_branches", "a cut without a state");
    if (misaligned(voxels, 3) || misaligned(nbrs, 3) || misaligned(state, 3) || misaligned(cut, 3) || misaligned(first, 3) || misaligned(branches, 7))
        return cvx_fail("trace_branches", "misaligned pointer");
    if (B > 0) CVX_HIP(hipMemsetAsync(branches, 0, (size_t)B * kBC * sizeof(int64_t), st));  // a B above the keys' count leaves zero rows
    hipLaunchKernelGGL(k_trace_rows, dim3(blocks_of(N)), dim3(kCclThreads), 0, st, voxels, nbrs, (const TraceState*)state, cut, first, H, W, N, B,
                       (long long*)branches);
    if (const int rc = cvx_check_launch()) return rc;
    if (B == 0) return 0;
    hipLaunchKernelGGL(k_trace_d2, dim3(blocks_of(N)), dim3(kCclThreads), 0, st, (const int32_t*)voxels, N, B, (long long*)branches);
    return cvx_check_launch();
}
