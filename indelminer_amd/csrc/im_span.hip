// im_span.hip -- reference-spanning read counts for the genotype columns (-G) on gfx950.
//
// There is no reference counterpart: the reference prints NS= (reads that support the indel) and nothing that counts the
// reads that support the REFERENCE allele at the same breakpoint.  The statistic, per contig of length clen and flank m >= 1:
//   a record is eligible iff its flag has none of 0x4 / 0x100 / 0x200 / 0x400 (the pileup's mask, as in im_triage.hip), its
//   tid names a contig and its mapping quality is >= min_mapq;
//   a RUN is a maximal sequence of consecutive M / = / X operations of its CIGAR, covering [s, e) clipped to [0, clen)
//   (D and N advance the position and end a run; every other operation ends a run without advancing);
//   span[p], 0 <= p <= clen, counts the runs with s <= p - m and p + m <= e: m matched bases on each side of the boundary in
//   front of base p.  As a difference array a run with e - s >= 2 m adds +1 at s + m and -1 at e - m + 1 (<= clen as m >= 1).
// The array has the depth array's layout (im_depth.hip): per contig clen + 1 entries, scanned by the same tiled scan.
//   span_scatter   one lane per delivered record: runs -> events, gathered in an LDS window, written out with vector atomics
//   (scan)         launch_depth_scan_tiled, as it is
//   span_query     one wave per query: minimum of span[p] over [beg, end] inclusive
// The record-at-a-time path hands over (start, length) runs instead of records: launch_depth_build(lo = m, hi = m - 1) makes the
// same events from them.

#include "im_device.hpp"

namespace im {
namespace {

constexpr int kSpanBlock = 256;
constexpr int kSpanWin = 4096;      // positions of the difference array a workgroup gathers in LDS before it touches memory
constexpr int kSpanHead = 4;        // CIGAR words a lane keeps in registers; the rest come from memory

__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }

// What the scatter needs of a record (the 32-byte core; layout as in include/indelminer_amd.h, im_dev_records)
struct SpanRec {
    const uint8_t* p;
    int32_t tid, pos;
    uint32_t mapq, n_cigar, flag, o_cigar;
    uint32_t cig[kSpanHead];
    bool ok;
};

__device__ __forceinline__ SpanRec span_record(const uint8_t* raw, uint32_t off, uint32_t end)
{
    SpanRec r;
    r.p = raw + off; r.ok = false; r.tid = -1; r.pos = 0; r.mapq = r.n_cigar = r.flag = r.o_cigar = 0;
#pragma unroll
    for (int k = 0; k < kSpanHead; k++) r.cig[k] = 0;
    if (end < off || end - off < 32u) return r;
    const uint32_t len = end - off;
    const uint32_t* c = reinterpret_cast<const uint32_t*>(r.p);     // 4-byte aligned by contract
    r.tid = (int32_t)c[0]; r.pos = (int32_t)c[1];
    const uint32_t w2 = c[2], w3 = c[3];
    r.mapq = (w2 >> 8) & 255u;
    r.n_cigar = w3 & 0xFFFFu; r.flag = w3 >> 16;
    r.o_cigar = 32u + (w2 & 255u);
    if ((uint64_t)r.o_cigar + 4ull * r.n_cigar > len) return r;     // the CIGAR lies inside the record
    r.ok = true;
    return r;
}

__device__ __forceinline__ uint32_t span_cigar_word(const SpanRec& r, uint32_t k)
{
    return k == 0u ? r.cig[0] : k == 1u ? r.cig[1] : k == 2u ? r.cig[2] : k == 3u ? r.cig[3] : ld_u32(r.p + r.o_cigar + 4u * k);
}

struct SpanArgs {
    im_dev_records recs;
    const int64_t* asc_off;     // [n_contigs] start of a contig's run in the array
    const int32_t* len;         // [n_contigs]
    int32_t n_contigs;
    int32_t flank, min_mapq;
    int32_t* diff;              // the genome-wide difference array
};

// one event of a run: into the LDS window when it lies there, to memory otherwise
__device__ __forceinline__ void span_event(int32_t* s_win, int32_t* __restrict__ diff, int64_t base, bool here, int64_t win_pos, int64_t at, int32_t v)
{
    const int64_t rel = at - win_pos;
    if (here && rel >= 0 && rel < kSpanWin) atomicAdd(&s_win[rel], v);
    else atomicAdd(&diff[base + at], v);
}

__global__ __launch_bounds__(kSpanBlock) void span_scatter_kernel(SpanArgs A)
{
    // A coordinate-sorted BAM puts the 256 records of a workgroup within a few hundred positions of each other: their events
    // become LDS adds and a few whole-line atomic instructions (the depth events of im_triage.hip's classify kernel take the
    // same road).  Events outside the window or on another contig go to memory directly.
    __shared__ int32_t s_win[kSpanWin];
    __shared__ int32_t s_wpos[kSpanBlock / 64], s_wtid[kSpanBlock / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i = (int64_t)blockIdx.x * kSpanBlock + t;
    {
        int4* z = reinterpret_cast<int4*>(s_win);
#pragma unroll
        for (int k = 0; k < kSpanWin / 4 / kSpanBlock; k++) z[t + k * kSpanBlock] = make_int4(0, 0, 0, 0);
    }
    SpanRec r; r.ok = false; r.tid = -1; r.pos = 0; r.flag = 0; r.mapq = 0; r.n_cigar = 0; r.o_cigar = 0; r.p = A.recs.raw;
    if (i < A.recs.n) r = span_record(A.recs.raw, A.recs.rec_off[i], A.recs.rec_off[i + 1]);
    if (r.ok) {
        // reads past the record stay inside the chunk buffer (>= 64 spare bytes behind the last record)
#pragma unroll
        for (int k = 0; k < kSpanHead; k++) r.cig[k] = ld_u32(r.p + r.o_cigar + 4u * k);
    }
    const bool counts = r.ok && r.tid >= 0 && r.tid < A.n_contigs && !(r.flag & (0x4u | 0x100u | 0x200u | 0x400u)) && (int32_t)r.mapq >= A.min_mapq;
    // the window starts at the first eligible record of the workgroup (records are sorted inside a contig)
    {
        const uint64_t mp = __ballot(counts);
        const int first = mp ? (int)__builtin_ctzll(mp) : 0;
        const int fp = __shfl(r.pos, first), ft = __shfl(r.tid, first);
        if (lane == 0) { s_wpos[wave] = fp < 0 ? 0 : fp; s_wtid[wave] = mp ? ft : -1; }
    }
    __syncthreads();
    int32_t win_pos = 0, win_tid = -1;
#pragma unroll
    for (int wv = kSpanBlock / 64 - 1; wv >= 0; wv--) if (s_wtid[wv] >= 0) { win_tid = s_wtid[wv]; win_pos = s_wpos[wv]; }
    if (win_tid < 0) return;                                        // nothing eligible in the whole workgroup

    if (counts) {
        const int64_t base = A.asc_off[r.tid];
        const int64_t clen = A.len[r.tid], m = A.flank;
        const bool here = r.tid == win_tid;
        int64_t x = r.pos, rs = 0;
        bool in_run = false;
        for (uint32_t k = 0; k <= r.n_cigar; k++) {
            // one step behind the last operation closes the run that is open
            const uint32_t cw = k < r.n_cigar ? span_cigar_word(r, k) : 4u /* 0S */, op = cw & 15u;
            const int64_t len = cw >> 4;
            if (op == 0u || op == 7u || op == 8u) {
                if (!in_run) { rs = x; in_run = true; }
                x += len;
                continue;
            }
            if (in_run) {
                const int64_t a = rs < 0 ? 0 : rs, b = x > clen ? clen : x;
                if (b - a >= 2 * m) {
                    span_event(s_win, A.diff, base, here, win_pos, a + m, 1);
                    span_event(s_win, A.diff, base, here, win_pos, b - m + 1, -1);
                }
                in_run = false;
            }
            if (op == 2u || op == 3u) x += len;
        }
    }
    __syncthreads();
    // the gathered window out: consecutive lanes hold consecutive positions, only non-zero entries touch memory
    int32_t* dst = A.diff + A.asc_off[win_tid] + win_pos;
    const int64_t room = (int64_t)A.len[win_tid] + 1 - win_pos;    // the contig's run has len + 1 entries
#pragma unroll 4
    for (int k = 0; k < kSpanWin / kSpanBlock; k++) {
        const int idx = t + k * kSpanBlock;
        const int32_t v = s_win[idx];
        if (v != 0 && idx < room) atomicAdd(&dst[idx], v);
    }
}

// One wave per query: the minimum of span[p] over [beg, end] INCLUSIVE, clipped to [0, clen]; an interval that is empty after
// the clip answers 0.  sums: the tile offsets of the tiled scan.
__global__ __launch_bounds__(256) void span_query_kernel(int32_t nq, const int32_t* __restrict__ beg, const int32_t* __restrict__ end,
                                                        const int32_t* __restrict__ span, const int32_t* __restrict__ sums,
                                                        int64_t clen, uint32_t* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < nq; q += nwaves) {
        int64_t a = beg[q], b = end[q];
        if (a < 0) a = 0;
        if (b > clen) b = clen;
        uint32_t mn = 0xFFFFFFFFu;
        for (int64_t p = a + lane; p <= b; p += 64) mn = min(mn, (uint32_t)(span[p] + sums[p / kScanTile]));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, o));
        if (lane == 0) out[q] = a <= b ? mn : 0u;
    }
}

}  // namespace

hipError_t launch_span_scatter(const RefDev& ref, int32_t flank, int32_t min_mapq, const im_dev_records& recs, int32_t* diff, hipStream_t stream)
{
    if (recs.n <= 0) return hipSuccess;
    SpanArgs A;
    A.recs = recs; A.asc_off = ref.asc_off; A.len = ref.len; A.n_contigs = ref.n_contigs;
    A.flank = flank; A.min_mapq = min_mapq; A.diff = diff;
    const int blocks = (recs.n + kSpanBlock - 1) / kSpanBlock;
    hipLaunchKernelGGL(span_scatter_kernel, dim3(blocks), dim3(kSpanBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_span_query(int32_t nq, const int32_t* beg, const int32_t* end, const int32_t* span, const int32_t* sums,
                             int64_t clen, uint32_t* out, hipStream_t stream)
{
    if (nq <= 0) return hipSuccess;
    int b = (nq + 3) / 4;
    if (b > 2048) b = 2048;
    hipLaunchKernelGGL(span_query_kernel, dim3(b), dim3(256), 0, stream, nq, beg, end, span, sums, clen, out);
    return hipGetLastError();
}

}  // namespace im
