// im_depth.hip -- the per-contig difference array on gfx950: region depth for the DP= field, and the build and scan that
// the reference-spanning counts (im_span.hip) share with it.
//
// Replaces calculate_cov_params (src/shared.c:151-212), which re-opens the BAM, reloads the
// whole index and runs a samtools pileup for EVERY printed variant.  Pileup semantics kept
// (bam_pileup.c:67-143,238-265): a position counts a read iff the read passes
// the default mask (unmapped / secondary / QC-fail / duplicate are skipped) and its covering
// CIGAR op is M, = or X.  An array is clen + 1 int32 of one contig and goes through three steps:
//   scatter             +1 / -1 events into the zeroed array (device atomics): depth_scatter here for host-given intervals
//                       (the build forms, for callers that name the events themselves; the host driver's record-at-a-time path
//                       uses the depth one), im_triage.hip / im_span.hip from the records for the genome-wide arrays
//   depth_scan_tiled    ONE launch: prefix sum inside tiles of 8192 positions, a tile per workgroup of 256 lanes with the whole tile
//                       in flight; the workgroup that arrives last turns the tiles' totals into exclusive tile offsets in sums[].
//                       The array stays tile-local (HBM streaming, one pass)
//   depth_query_tiled   one wave per printed variant: sum of data[p] + sums[p / 8192] over [start-lw-1, stop+rw+1)
// The host takes floor(sum / length) like the reference (src/shared.c:205).
//
// sums[], ONE rule for every array (one contig's or a run of the genome-wide ones): depth_sums_ints(clen) ints -- the tiles'
// totals, then the arrival counter of the groups, then one arrival counter per group of kScanGroup tiles.  The counters are
// zero whenever a scan starts.  The scan leaves them zero, so an array that is always scanned at one clen (a contig's run of
// the genome-wide arrays) is zeroed once, when it is allocated.  An array that serves contigs of different lengths
// (launch_depth_build) has a longer contig's tile offsets where a shorter one's counters lie: every build zeroes its sums.

#include "im_device.hpp"

namespace im {
namespace {

constexpr int kScanBlock = 256;
constexpr int kScanItems = 8;                               // a lane's share of one sub-tile: two 16-byte accesses
constexpr int kScanSub = kScanBlock * kScanItems;           // positions of a sub-tile: a wave reads 2 KB of it in one piece
constexpr int kScanSubs = kScanTile / kScanSub;             // sub-tiles of a tile, all with one workgroup
constexpr int kScanWaves = kScanBlock / 64;
static_assert(kScanTile == kScanSub * kScanSubs, "im_device.hpp names the tile for the queries");
constexpr int kScanGroup = 32;      // tiles that count their arrival into one word (depth_scan_tiled_kernel)
constexpr int kOffItems = 4;        // tile totals a lane of the last workgroup takes per round of the offset pass

// host-given intervals [start, start + len) of one contig, clipped to [0, clen): +1 at a + lo, -1 at b - hi iff a + lo < b - hi
// (launch_depth_build has the two uses)
__global__ __launch_bounds__(256) void depth_scatter_kernel(int32_t n_seg, const int32_t* __restrict__ start, const int32_t* __restrict__ len,
                                                           int64_t clen, int64_t lo, int64_t hi, int32_t* __restrict__ diff)
{
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_seg; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t a = start[i], b = (int64_t)start[i] + len[i];
        if (a < 0) a = 0;
        if (b > clen) b = clen;
        if (a + lo >= b - hi) continue;
        atomicAdd(&diff[a + lo], 1);
        atomicAdd(&diff[b - hi], -1);
    }
}

// One tile's inclusive scan, in place.  A lane holds kScanItems consecutive positions of each of the tile's kScanSubs sub-tiles;
// every load of the tile is issued before the first is consumed (128 bytes in flight per lane, the whole tile per workgroup).
// One barrier: the kScanSubs x kScanWaves wave totals meet in LDS, and every lane adds up the ones in front of it.
// Whole: the tile lies inside [0, n) and travels as 16-byte accesses (the contig's run starts on a 256-byte boundary);
// otherwise position by position, a clamped index instead of a branch around each load.  Lane 0 sends the tile's total to *total
// in front of the tile's stores, so that its round trip runs beside them; returns what that atomic returned.
template <bool Whole>
__device__ __forceinline__ int32_t scan_tile(int32_t* __restrict__ data, int64_t n, int64_t tile0, int32_t* wsum, int tid, int32_t* total)
{
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int32_t v[kScanSubs][kScanItems];
    static_assert(kScanItems == 8, "a lane's eight items travel as two 16-byte accesses");
    data += tile0;                                          // positions of the tile from here on: 32-bit offsets from a uniform base
    const int32_t room = (int32_t)(n - tile0 < kScanTile ? n - tile0 : kScanTile);      // >= 1: the tile exists
#pragma unroll
    for (int s = 0; s < kScanSubs; s++) {
        const int32_t base = s * kScanSub + tid * kScanItems;
        if (Whole) {
            const int4 a = *reinterpret_cast<const int4*>(data + base), c = *reinterpret_cast<const int4*>(data + base + 4);
            v[s][0] = a.x; v[s][1] = a.y; v[s][2] = a.z; v[s][3] = a.w; v[s][4] = c.x; v[s][5] = c.y; v[s][6] = c.z; v[s][7] = c.w;
        } else {
#pragma unroll
            for (int e = 0; e < kScanItems; e++) { const int32_t i = base + e, t = data[i < room ? i : room - 1]; v[s][e] = i < room ? t : 0; }
        }
    }
    int32_t run[kScanSubs], x[kScanSubs];
#pragma unroll
    for (int s = 0; s < kScanSubs; s++) {
        int32_t r = 0;
#pragma unroll
        for (int e = 0; e < kScanItems; e++) { r += v[s][e]; v[s][e] = r; }
        run[s] = x[s] = r;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int s = 0; s < kScanSubs; s++) { const int32_t t = __shfl_up(x[s], o); if (lane >= o) x[s] += t; }
    }
    if (lane == 63) {
#pragma unroll
        for (int s = 0; s < kScanSubs; s++) wsum[s * kScanWaves + wave] = x[s];
    }
    __syncthreads();
    int32_t pre = 0, front[kScanSubs];
#pragma unroll
    for (int s = 0; s < kScanSubs; s++) {
#pragma unroll
        for (int w = 0; w < kScanWaves; w++) { if (w == wave) front[s] = pre; pre += wsum[s * kScanWaves + w]; }
    }
    int32_t seen = 0;
    if (tid == 0) seen = atomicExch(total, pre);
#pragma unroll
    for (int s = 0; s < kScanSubs; s++) {
        const int32_t base = s * kScanSub + tid * kScanItems;
        const int32_t excl = front[s] + x[s] - run[s];
        if (Whole) {
            *reinterpret_cast<int4*>(data + base) = make_int4(v[s][0] + excl, v[s][1] + excl, v[s][2] + excl, v[s][3] + excl);
            *reinterpret_cast<int4*>(data + base + 4) = make_int4(v[s][4] + excl, v[s][5] + excl, v[s][6] + excl, v[s][7] + excl);
        } else {
#pragma unroll
            for (int e = 0; e < kScanItems; e++) if (base + e < room) data[base + e] = v[s][e] + excl;
        }
    }
    return seen;
}

// ONE launch per contig: an inclusive scan inside each tile of 8192 elements, and the workgroup that finishes last turns the tile totals
// into exclusive offsets in place.  The depths are left tile-local; depth_query_tiled adds a position's tile offset when it
// reads it -- no third pass over the contig.  No workgroup waits for another: the one that arrives last does the extra work, every
// other one leaves.  Totals travel through returning agent-scope atomics (written and read back on the same path, no fence:
// im_triage.hip uses the same hand-over).  The arrival counters (sums[tiles] for the groups, then one per group) are zero between
// launches: they count with a wrapping increment, so the arrival that completes a count also puts the word back to zero and
// nothing is left to reset.  A tile's chain is its total, then its group's count; the tile that completes a group adds the groups' count.
__global__ __launch_bounds__(kScanBlock) void depth_scan_tiled_kernel(int32_t* __restrict__ data, int64_t n, int32_t* __restrict__ sums, int32_t tiles)
{
    __shared__ int32_t wsum[kScanSubs * kScanWaves];
    __shared__ int32_t osum[2][kScanWaves];
    __shared__ int32_t s_last;
    const int tid = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * kScanTile;
    const int32_t seen = tile0 + kScanTile <= n ? scan_tile<true>(data, n, tile0, wsum, tid, &sums[blockIdx.x])
                                                : scan_tile<false>(data, n, tile0, wsum, tid, &sums[blockIdx.x]);
    if (tid == 0) {
        asm volatile("" :: "v"(seen));                  // the total is in before this workgroup is counted
        // counted in two levels -- a group of kScanGroup tiles, then the groups: same-address atomics are served one after the
        // other (~9 ns each: 7 us of the 6.25 Mb contig's launch when every tile counted into one word, im_triage.hip has the measurement)
        const int32_t g = (int32_t)blockIdx.x / kScanGroup, groups = (tiles + kScanGroup - 1) / kScanGroup;
        const uint32_t g_n = (uint32_t)min(kScanGroup, tiles - g * kScanGroup);
        bool last = atomicInc(reinterpret_cast<uint32_t*>(&sums[tiles + 1 + g]), g_n - 1u) == g_n - 1u;
        if (last && groups > 1) last = atomicInc(reinterpret_cast<uint32_t*>(&sums[tiles]), (uint32_t)groups - 1u) == (uint32_t)groups - 1u;
        s_last = last ? 1 : 0;
    }
    __syncthreads();
    if (!s_last) return;
    // the offset pass: kScanBlock * kOffItems tiles a round, one barrier a round (the waves' sums alternate between two rows of
    // osum; the running offset stays in registers).  The totals are read with agent-scope atomic loads, behind the barrier that
    // follows the last count's return -- the instruction an atomicAdd(p, 0) becomes -- all of a round in flight at once and
    // no branch around any of them (a clamped index instead).
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int32_t carry = 0;
    for (int32_t b0 = 0, row = 0; b0 < tiles; b0 += kScanBlock * kOffItems, row ^= 1) {
        const int32_t j0 = b0 + tid * kOffItems;
        int32_t t[kOffItems];
#pragma unroll
        for (int k = 0; k < kOffItems; k++) {
            const int32_t j = j0 + k, u = __hip_atomic_load(&sums[j < tiles ? j : tiles - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            t[k] = j < tiles ? u : 0;
        }
        int32_t r = 0;
#pragma unroll
        for (int k = 0; k < kOffItems; k++) { const int32_t u = t[k]; t[k] = r; r += u; }
        int32_t y = r;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int32_t u = __shfl_up(y, o); if (lane >= o) y += u; }
        if (lane == 63) osum[row][wave] = y;
        __syncthreads();
        int32_t front = carry;
#pragma unroll
        for (int w = 0; w < kScanWaves; w++) { if (w == wave) front = carry; carry += osum[row][w]; }
        const int32_t excl = front + y - r;
#pragma unroll
        for (int k = 0; k < kOffItems; k++) if (j0 + k < tiles) sums[j0 + k] = excl + t[k];
    }
}

__global__ __launch_bounds__(256) void depth_query_tiled_kernel(int32_t nq, const int32_t* __restrict__ beg, const int32_t* __restrict__ end,
                                                               const int32_t* __restrict__ depth, const int32_t* __restrict__ sums,
                                                               int64_t clen, uint32_t* __restrict__ out, uint32_t* __restrict__ out_max)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < nq; q += nwaves) {
        int64_t a = beg[q], b = end[q];
        if (a < 0) a = 0;
        if (b > clen) b = clen;
        // out_max: the deepest position of [beg - 1, end] (the host asks the file about loci deep enough for samtools' pileup cap)
        const int64_t a1 = out_max && a > 0 ? a - 1 : a, b1 = out_max && b < clen ? b + 1 : b;
        uint32_t s = 0, mx = 0;
        for (int64_t p = a1 + lane; p < b1; p += 64) {
            const uint32_t v = (uint32_t)(depth[p] + sums[p / kScanTile]);
            if (p >= a && p < b) s += v;
            mx = max(mx, v);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { s += (uint32_t)__shfl_xor((int)s, o); mx = max(mx, (uint32_t)__shfl_xor((int)mx, o)); }
        if (lane == 0) { out[q] = s; if (out_max) out_max[q] = mx; }
    }
}

// ---- the median of a scanned array over an interval (im_depth_median, im_depth_median_tid) ----------------------------------
// Lower median of v[p] = min(data[p] + sums[p / kScanTile], kMedBins - 1) over the positions of [beg, end) clipped to [0, clen):
// the smallest d with at least (n + 1) / 2 of the n positions at v <= d.  By histogram: kMedBins counters of 32 bits in LDS.
// An interval is cut into slabs of kMedSlab positions from its first position rounded down to a multiple of 4 (so that every lane's
// four positions are one 16-byte access and lie in one scan tile); a slab is one work item of a workgroup of 256 lanes, the
// work items of a call are numbered query by query (first[q] .. first[q + 1]) and the workgroups take them grid-stride.
//   one slab      the workgroup picks the median from its LDS histogram and is done
//   several       every slab adds its non-zero bins to the query's histogram in device memory (g_hist, returning agent-scope
//                 atomics, every access to that memory is one) and counts its arrival with a wrapping increment; the slab that
//                 arrives last takes the bins out with exchanges against zero and picks.  Bins and counter are zero again
//                 behind it: nothing to reset between calls.  Order: every lane consumes the returns of its adds, a barrier,
//                 then lane 0 counts behind an agent-scope release fence; the last arriver passes an acquire fence before its
//                 lanes read.  depth_scan_tiled_kernel relies on the consumed returns alone; here the fences make the pairing
//                 formal, so it does not hang on where the compiler places a wait (about 2 us per slab of such a query).
// LDS form: a lane folds the equal neighbours among its four consecutive positions into one ds_add of the run's length (depth
// moves at read ends only: most quads are one run, a quarter of the atomics), and nothing is combined across lanes.  A wave-wide
// combination would need a 64-lane match per instruction, which gfx950 has no instruction for; neither form has been measured.
constexpr int kMedBins = 4096;
constexpr int kMedSlab = 4 * kScanTile;                     // positions of a slab: 128 KB of the array
constexpr int kMedBlock = 256;
constexpr int kMedAhead = 4;                                // 16-byte loads a lane has in flight in front of the LDS atomics
constexpr int kMedSegs = kMedBins / (kMedBlock * 4);        // a lane holds 4 consecutive bins of each of these segments of the histogram
constexpr int kMedWaves = kMedBlock / 64;
constexpr int kMedTiles = kMedSlab / kScanTile + 1;         // scan tiles a slab can touch (it starts anywhere in one)
static_assert(kMedSegs * kMedBlock * 4 == kMedBins && kMedSlab % kScanTile == 0 && kMedSlab % (4 * kMedBlock * kMedAhead) == 0, "");

__device__ __forceinline__ uint32_t med_bin(int32_t v) { return min((uint32_t)v, (uint32_t)(kMedBins - 1)); }

// four consecutive positions into the histogram: one add per run of equal values
__device__ __forceinline__ void med_add_quad(uint32_t* hist, const int4 v, int32_t off)
{
    const uint32_t d0 = med_bin(v.x + off), d1 = med_bin(v.y + off), d2 = med_bin(v.z + off), d3 = med_bin(v.w + off);
    uint32_t run = 1;
    if (d1 == d0) run++; else { atomicAdd(&hist[d0], run); run = 1; }
    if (d2 == d1) run++; else { atomicAdd(&hist[d1], run); run = 1; }
    if (d3 == d2) run++; else { atomicAdd(&hist[d2], run); run = 1; }
    atomicAdd(&hist[d3], run);
}

__global__ __launch_bounds__(kMedBlock) void depth_median_kernel(int32_t nq, const int32_t* __restrict__ beg, const int32_t* __restrict__ end,
                                                                 const int32_t* __restrict__ first, const int32_t* __restrict__ slot,
                                                                 const int32_t* __restrict__ data, const int32_t* __restrict__ sums, int64_t clen,
                                                                 uint32_t* __restrict__ g_hist, uint32_t* __restrict__ g_count, uint32_t* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist[kMedBins];
    __shared__ int32_t s_tsum[kMedTiles];
    __shared__ uint32_t wsum[kMedSegs * kMedWaves];
    __shared__ int32_t s_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
    for (int s = 0; s < kMedSegs; s++) reinterpret_cast<uint4*>(hist)[s * kMedBlock + tid] = make_uint4(0, 0, 0, 0);
    const int32_t w_first = first[0], items = first[nq] - w_first;
    for (int32_t w = blockIdx.x; w < items; w += gridDim.x) {
        // the query of this work item: first[q] <= w_first + w < first[q + 1] (queries without positions have no items)
        const int32_t wabs = w_first + w;
        int32_t q = 0;
        for (int32_t hi = nq; hi - q > 1;) { const int32_t mid = (q + hi) >> 1; if (first[mid] <= wabs) q = mid; else hi = mid; }
        int64_t a = beg[q], b = end[q];
        if (a < 0) a = 0;
        if (b > clen) b = clen;                                     // a < b: the query has items
        const int32_t nslab = first[q + 1] - first[q];
        const int64_t s0 = (a & ~(int64_t)3) + (int64_t)(wabs - first[q]) * kMedSlab;       // a multiple of 4
        const int64_t s1 = s0 + kMedSlab < b ? s0 + kMedSlab : b, lo = a > s0 ? a : s0;     // the slab's positions are [lo, s1)
        const int32_t r0 = (int32_t)(s0 % kScanTile);
        if (tid < kMedTiles) { const int64_t t = s0 / kScanTile + tid, tl = (b - 1) / kScanTile; s_tsum[tid] = sums[t < tl ? t : tl]; }
        __syncthreads();                                            // the tile offsets are in, the histogram is zero
        const int32_t* __restrict__ base = data + s0;               // 32-bit offsets from a uniform base from here on
        // whole quads [body_lo, body_hi) of the slab, kMedAhead 16-byte loads of a lane issued before the first is consumed; a
        // clamped index instead of a branch around a load
        const int32_t body_lo = (int32_t)(((lo + 3) & ~(int64_t)3) - s0), body_hi = (int32_t)(s1 - s0) & ~3;
        const int32_t nquad = body_hi > body_lo ? (body_hi - body_lo) >> 2 : 0;
        for (int32_t i0 = 0; i0 < nquad; i0 += kMedBlock * kMedAhead) {
            int4 v[kMedAhead];
            int32_t off[kMedAhead];
#pragma unroll
            for (int k = 0; k < kMedAhead; k++) {
                const int32_t i = i0 + k * kMedBlock + tid, o = body_lo + 4 * (i < nquad ? i : nquad - 1);
                v[k] = *reinterpret_cast<const int4*>(base + o);
                off[k] = s_tsum[(r0 + o) / kScanTile];
            }
#pragma unroll
            for (int k = 0; k < kMedAhead; k++) if (i0 + k * kMedBlock + tid < nquad) med_add_quad(hist, v[k], off[k]);
        }
        // the positions in front of the first whole quad (lanes 0..3) and behind the last (lanes 4..7), one each
        if (tid < 8) {
            const int32_t o = tid < 4 ? body_lo - 4 + tid : (body_hi > body_lo ? body_hi : body_lo) + tid - 4;
            const int64_t p = s0 + o, stop = tid < 4 && s0 + body_lo < s1 ? s0 + body_lo : s1;
            if (p >= lo && p < stop) atomicAdd(&hist[med_bin(base[o] + s_tsum[(r0 + o) / kScanTile])], 1u);
        }
        __syncthreads();                                            // the slab's histogram is complete
        uint32_t c[kMedSegs][4];
#pragma unroll
        for (int s = 0; s < kMedSegs; s++) {
            const uint4 t = reinterpret_cast<const uint4*>(hist)[s * kMedBlock + tid];
            reinterpret_cast<uint4*>(hist)[s * kMedBlock + tid] = make_uint4(0, 0, 0, 0);       // for the next work item
            c[s][0] = t.x; c[s][1] = t.y; c[s][2] = t.z; c[s][3] = t.w;
        }
        if (nslab > 1) {
            uint32_t* __restrict__ gh = g_hist + (size_t)slot[q] * kMedBins;
            uint32_t seen = 0;
#pragma unroll
            for (int s = 0; s < kMedSegs; s++) {
#pragma unroll
                for (int e = 0; e < 4; e++) if (c[s][e]) seen |= atomicAdd(&gh[(s * kMedBlock + tid) * 4 + e], c[s][e]);
            }
            asm volatile("" :: "v"(seen));                          // this lane's adds are in before the barrier in front of the count
            __syncthreads();
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // the workgroup's adds happen before its count ...
                const bool last = atomicInc(&g_count[slot[q]], (uint32_t)nslab - 1u) == (uint32_t)nslab - 1u;
                if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");       // ... and every count before the last arriver's reads
                s_last = last ? 1 : 0;
            }
            __syncthreads();
            if (!s_last) continue;                                  // uniform: every lane reads the same word
#pragma unroll
            for (int s = 0; s < kMedSegs; s++) {
#pragma unroll
                for (int e = 0; e < 4; e++) c[s][e] = atomicExch(&gh[(s * kMedBlock + tid) * 4 + e], 0u);
            }
        }
        // the pick: bins in the order segment, lane, element; a wave scan per segment, the waves' totals meet in LDS behind one barrier
        uint32_t run[kMedSegs], x[kMedSegs];
#pragma unroll
        for (int s = 0; s < kMedSegs; s++) run[s] = x[s] = c[s][0] + c[s][1] + c[s][2] + c[s][3];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
            for (int s = 0; s < kMedSegs; s++) { const uint32_t t = (uint32_t)__shfl_up((int)x[s], o); if (lane >= o) x[s] += t; }
        }
        if (lane == 63) {
#pragma unroll
            for (int s = 0; s < kMedSegs; s++) wsum[s * kMedWaves + wave] = x[s];
        }
        __syncthreads();
        const uint32_t want = (uint32_t)((b - a + 1) / 2);          // 1 <= want <= b - a = the sum of all bins: exactly one bin is the answer
        uint32_t pre = 0;
#pragma unroll
        for (int s = 0; s < kMedSegs; s++) {
            uint32_t front = 0;
#pragma unroll
            for (int k = 0; k < kMedWaves; k++) { if (k == wave) front = pre; pre += wsum[s * kMedWaves + k]; }
            uint32_t acc = front + x[s] - run[s];
            if (acc < want && want <= acc + run[s]) {
                int e = 0;
                for (; e < 3; e++) { acc += c[s][e]; if (acc >= want) break; }
                out[q] = (uint32_t)((s * kMedBlock + tid) * 4 + e);
            }
        }
        // wsum is read above and written behind the next work item's two barriers; s_tsum and s_last likewise
    }
}

// zeroes n ints from p (16-byte aligned): 16-byte stores, the up to three ints behind them by the first lanes of workgroup 0 -- one launch
constexpr int kFillBlock = 256;
__global__ __launch_bounds__(kFillBlock) void fill_zero_kernel(int32_t* p, int64_t n)
{
    const int64_t quads = n / 4;
    int4* q = reinterpret_cast<int4*>(p);
    const int64_t stride = (int64_t)gridDim.x * kFillBlock;
    for (int64_t k = (int64_t)blockIdx.x * kFillBlock + threadIdx.x; k < quads; k += stride) q[k] = make_int4(0, 0, 0, 0);
    if (blockIdx.x == 0 && 4 * quads + threadIdx.x < n) p[4 * quads + threadIdx.x] = 0;
}

}  // namespace

// A contig's run of a counted array back to zero (im_*_reset): one launch of our own.  A hipMemsetAsync of a run whose
// length is not a multiple of the runtime's fill width came out as two dispatches per call (profiles/README.md).
// p is 16-byte aligned: a contig's run starts at a multiple of 256 ints of a hipMalloc'ed array (im_set_reference).
hipError_t launch_fill_zero(int32_t* p, int64_t n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (reinterpret_cast<uintptr_t>(p) & 15u) return hipErrorInvalidValue;
    int64_t b = (n / 4 + 4 * kFillBlock - 1) / (4 * kFillBlock);       // four 16-byte stores per lane
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    hipLaunchKernelGGL(fill_zero_kernel, dim3((int)b), dim3(kFillBlock), 0, stream, p, n);
    return hipGetLastError();
}

int64_t depth_sums_ints(int64_t clen) { const int64_t t = (clen + 1 + kScanTile - 1) / kScanTile; return t + 1 + (t + kScanGroup - 1) / kScanGroup; }

// difference array -> tile-local prefix sums + tile offsets, in place: n elements, sums as the header says for clen = n - 1
hipError_t launch_depth_scan_tiled(int32_t* depth, int64_t n, int32_t* sums, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const int64_t tiles = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(depth_scan_tiled_kernel, dim3((int)tiles), dim3(kScanBlock), 0, stream, depth, n, sums, (int32_t)tiles);
    return hipGetLastError();
}

// One contig's array from host-given intervals, scanned: data holds clen + 1 ints, sums depth_sums_ints(clen).
// The depth array is lo = hi = 0 (+1 at a, -1 at b iff a < b); the span array of flank m is lo = m, hi = m - 1
// (+1 at a + m, -1 at b - m + 1 iff b - a >= 2 m, im_span.hip).  0 <= lo, 0 <= hi: every event lies in [0, clen].
hipError_t launch_depth_build(int64_t clen, int32_t n_seg, const int32_t* seg_start, const int32_t* seg_len, int32_t lo, int32_t hi,
                              int32_t* data, int32_t* sums, hipStream_t stream)
{
    const int64_t n = clen + 1;
    hipError_t e = hipMemsetAsync(data, 0, (size_t)n * sizeof(int32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(sums, 0, (size_t)depth_sums_ints(clen) * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    if (n_seg > 0) {
        int64_t b = ((int64_t)n_seg + 255) / 256;
        if (b > 4096) b = 4096;
        hipLaunchKernelGGL(depth_scatter_kernel, dim3((int)b), dim3(256), 0, stream, n_seg, seg_start, seg_len, clen, (int64_t)lo, (int64_t)hi, data);
    }
    return launch_depth_scan_tiled(data, n, sums, stream);
}

hipError_t launch_depth_query_tiled(int32_t nq, const int32_t* beg, const int32_t* end, const int32_t* depth, const int32_t* sums,
                                    int64_t clen, uint32_t* out, uint32_t* out_max, hipStream_t stream)
{
    if (nq <= 0) return hipSuccess;
    int b = (nq + 3) / 4;
    if (b > 2048) b = 2048;
    hipLaunchKernelGGL(depth_query_tiled_kernel, dim3(b), dim3(256), 0, stream, nq, beg, end, depth, sums, clen, out, out_max);
    return hipGetLastError();
}

// slabs (work items of depth_median_kernel) of the query [beg, end) of a contig of clen positions: 0 iff it is empty after the clip
int32_t depth_median_slabs(int32_t beg, int32_t end, int64_t clen)
{
    int64_t a = beg, b = end;
    if (a < 0) a = 0;
    if (b > clen) b = clen;
    if (a >= b) return 0;
    return (int32_t)((b - (a & ~(int64_t)3) + kMedSlab - 1) / kMedSlab);
}

size_t depth_median_scratch_bytes(int32_t slots) { return (size_t)slots * (kMedBins + 1) * sizeof(uint32_t); }

// nq queries of one contig whose work items are first[0] .. first[nq] (first[q + 1] - first[q] = depth_median_slabs of query q); slot[q]:
// which histogram of scratch a query of several slabs adds into (distinct, < slots; unused for the others).  scratch holds
// depth_median_scratch_bytes(slots) of zeros and is left that way.  out[q] is written for every query that has positions.
hipError_t launch_depth_median(int32_t nq, int32_t items, const int32_t* beg, const int32_t* end, const int32_t* first, const int32_t* slot,
                               const int32_t* data, const int32_t* sums, int64_t clen, uint32_t* scratch, int32_t slots, int32_t max_blocks,
                               uint32_t* out, hipStream_t stream)
{
    if (nq <= 0 || items <= 0) return hipSuccess;
    const int b = items < max_blocks ? items : max_blocks;
    hipLaunchKernelGGL(depth_median_kernel, dim3(b), dim3(kMedBlock), 0, stream, nq, beg, end, first, slot, data, sums, clen,
                       scratch, scratch + (size_t)slots * kMedBins, out);
    return hipGetLastError();
}

}  // namespace im
