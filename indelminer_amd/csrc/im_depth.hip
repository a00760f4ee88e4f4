// im_depth.hip -- the per-contig difference array on gfx950: region depth for the DP= field, and the build and scan that
// the reference-spanning counts (im_span.hip) share with it.
//
// Replaces calculate_cov_params (src/shared.c:151-212), which re-opens the BAM, reloads the
// whole index and runs a samtools pileup for EVERY printed variant.  Pileup semantics kept
// (bam_pileup.c:67-143,238-265): a position counts a read iff the read passes
// the default mask (unmapped / secondary / QC-fail / duplicate are skipped) and its covering
// CIGAR op is M, = or X.  An array is clen + 1 int32 of one contig and goes through three steps:
//   scatter             +1 / -1 events into the zeroed array (device atomics): depth_scatter here for host-given intervals
//                       (the record-at-a-time path), im_triage.hip / im_span.hip from the records for the genome-wide arrays
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

}  // namespace

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

}  // namespace im
