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
//   span_ends      one lane per end, each on its own contig: the same minimum over [pos - slack, pos + slack] (-K)
// The build form, for callers that name the events themselves, takes (start, length) runs instead of records:
// launch_depth_build(lo = m, hi = m - 1) makes the same events from them.
//
// Concordant pairs (-P), a second array of the same shape for the records without a precise breakpoint (PAIRED_READ).  With
// m = flank >= 1, q = min_mapq and range_max = range[1] of the record's read group (its RG:Z tag, "generic" without one: the
// look-up of fetch_func), a record is a CONCORDANT LEFT MATE iff
//   flag & 0x1, none of 0x4 | 0x8 | 0x100 | 0x200 | 0x400 | 0x800;  0 <= tid < n_contigs and mtid == tid;
//   ((flag >> 4) & 1) != ((flag >> 5) & 1)  (the orientation test of the discordant rule);  isize > 0;
//   pos < mpos, or pos == mpos and flag & 0x40  (each pair once);  mapq >= q;
//   its read group is in the table and isize <= range_max  (the complement of the evidence rule abs(isize) > range[1]; a record
//   whose group is not in the table is skipped: the triage of the same chunk ends the run on it).
// Its FRAGMENT is [a, b) = [pos, pos + isize) clipped to [0, clen).  pspan[p], 0 <= p <= clen, counts the fragments with
// a + m <= p and p + m <= b: a fragment with b - a >= 2 m adds +1 at a + m and -1 at b - m + 1.  Scan and query as for span[].
//   pair_scatter   one lane per delivered record: the core decides first, the survivors find RG:Z and look the group up (im_rg.hpp)
//
// Clipped reads (-C), two POINT-COUNT arrays of the same layout, never scanned.  A record is eligible as for span[] and when its
// CIGAR has at least one M / = / X / D / N.  `first` / `last`: its first / last operation that is not H; refend = pos + the
// lengths of its M / = / X / D / N operations.
//   clipR[refend] += 1  iff last is S of >= min_clip bases and 0 <= refend <= clen  (a read that stops aligning in front of refend)
//   clipL[pos] += 1     iff first is S of >= min_clip bases and 0 <= pos <= clen    (a read that starts aligning at pos)
// A record can add to both; an S anywhere else is not looked at here (the triage of the same chunk ends the run on it).
//   clip_scatter   one lane per delivered record: the core and two CIGAR words at either end decide, a right clip walks its CIGAR
//   clip_argmax    one wave per query: the largest count over [beg, end] inclusive and the smallest position that holds it
//   clip_facing    one lane per four positions of one contig: the facing piles of the two arrays (-I), the one chip-wide search
//   clip_peaks     the same stream over one array: its peaks (-U), once per side
// clip_build, for callers that name the events themselves, adds one per (position, side).

#include "im_device.hpp"
#include "im_rg.hpp"
#include "im_spanrec.hpp"

namespace im {
namespace {

constexpr int kSpanBlock = 256;
constexpr int kSpanWin = 4096;      // positions of the difference array a workgroup gathers in LDS before it touches memory
__device__ __forceinline__ uint32_t span_cigar_word(const SpanRec& r, uint32_t k)
{
    return k == 0u ? r.cig[0] : k == 1u ? r.cig[1] : k == 2u ? r.cig[2] : k == 3u ? r.cig[3] : ld_u32(r.p + r.o_cigar + 4u * k);
}

// what both scatter kernels take
struct ScatterArgs {
    im_dev_records recs;
    const int64_t* asc_off;     // [n_contigs] start of a contig's run in the array
    const int32_t* len;         // [n_contigs]
    int32_t n_contigs;
    int32_t flank, min_mapq;
    RgTable rg;                 // read group -> range[1] (im_set_insert_ranges); the pair kernel only
    int32_t* diff;              // the genome-wide difference array
};

// The LDS window of a scatter workgroup: kSpanWin positions of one contig's difference array, from the position of the first
// record of the workgroup that has events to add.  A coordinate-sorted BAM puts the 256 records of a workgroup within a few
// hundred positions of each other: their events become LDS adds and a few whole-line atomic instructions (the depth events of
// im_triage.hip's classify kernel take the same road).  Events outside the window or on another contig go to memory directly.
struct SpanWin { int32_t* lds; int32_t pos, tid; };

__device__ __forceinline__ void win_clear(int32_t* s_win, int t)
{
    int4* z = reinterpret_cast<int4*>(s_win);
#pragma unroll
    for (int k = 0; k < kSpanWin / 4 / kSpanBlock; k++) z[t + k * kSpanBlock] = make_int4(0, 0, 0, 0);
}

// each wave names its first record that adds events (records are sorted inside a contig); a __syncthreads, then win_open
__device__ __forceinline__ void win_propose(int32_t* s_wpos, int32_t* s_wtid, bool adds, int32_t pos, int32_t tid, int lane, int wave)
{
    const uint64_t mp = __ballot(adds);
    const int first = mp ? (int)__builtin_ctzll(mp) : 0;
    const int fp = __shfl(pos, first), ft = __shfl(tid, first);
    if (lane == 0) { s_wpos[wave] = fp < 0 ? 0 : fp; s_wtid[wave] = mp ? ft : -1; }
}

// the first wave with such a record decides; tid < 0: no record of the workgroup adds anything
__device__ __forceinline__ SpanWin win_open(int32_t* s_win, const int32_t* s_wpos, const int32_t* s_wtid)
{
    SpanWin W; W.lds = s_win; W.pos = 0; W.tid = -1;
#pragma unroll
    for (int wv = kSpanBlock / 64 - 1; wv >= 0; wv--) if (s_wtid[wv] >= 0) { W.tid = s_wtid[wv]; W.pos = s_wpos[wv]; }
    return W;
}

// one event on contig tid (base: the start of its run in diff): into the window when it lies there, to memory otherwise
__device__ __forceinline__ void win_event(const SpanWin& W, int32_t* __restrict__ diff, int64_t base, int32_t tid, int64_t at, int32_t v)
{
    const int64_t rel = at - W.pos;
    if (tid == W.tid && rel >= 0 && rel < kSpanWin) atomicAdd(&W.lds[rel], v);
    else atomicAdd(&diff[base + at], v);
}

// the gathered window out, behind a __syncthreads: consecutive lanes hold consecutive positions, only non-zero entries touch memory
__device__ __forceinline__ void win_out(const SpanWin& W, int32_t* __restrict__ diff, const int64_t* asc_off, const int32_t* len, int t)
{
    int32_t* dst = diff + asc_off[W.tid] + W.pos;
    const int64_t room = (int64_t)len[W.tid] + 1 - W.pos;          // the contig's run has len + 1 entries
#pragma unroll 4
    for (int k = 0; k < kSpanWin / kSpanBlock; k++) {
        const int idx = t + k * kSpanBlock;
        const int32_t v = W.lds[idx];
        if (v != 0 && idx < room) atomicAdd(&dst[idx], v);
    }
}

__global__ __launch_bounds__(kSpanBlock) void span_scatter_kernel(ScatterArgs A)
{
    __shared__ int32_t s_win[kSpanWin];
    __shared__ int32_t s_wpos[kSpanBlock / 64], s_wtid[kSpanBlock / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i = (int64_t)blockIdx.x * kSpanBlock + t;
    win_clear(s_win, t);
    SpanRec r; r.ok = false; r.tid = -1; r.pos = 0; r.flag = 0; r.mapq = 0; r.n_cigar = 0; r.o_cigar = 0; r.p = A.recs.raw;
    if (i < A.recs.n) r = span_record(A.recs.raw, A.recs.rec_off[i], A.recs.rec_off[i + 1]);
    if (r.ok) {
        // reads past the record stay inside the chunk buffer (>= 64 spare bytes behind the last record)
#pragma unroll
        for (int k = 0; k < kSpanHead; k++) r.cig[k] = ld_u32(r.p + r.o_cigar + 4u * k);
    }
    const bool counts = r.ok && r.tid >= 0 && r.tid < A.n_contigs && !(r.flag & (0x4u | 0x100u | 0x200u | 0x400u)) && (int32_t)r.mapq >= A.min_mapq;
    win_propose(s_wpos, s_wtid, counts, r.pos, r.tid, lane, wave);
    __syncthreads();
    const SpanWin W = win_open(s_win, s_wpos, s_wtid);
    if (W.tid < 0) return;                                          // nothing eligible in the whole workgroup

    if (counts) {
        const int64_t base = A.asc_off[r.tid];
        const int64_t clen = A.len[r.tid], m = A.flank;
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
                    win_event(W, A.diff, base, r.tid, a + m, 1);
                    win_event(W, A.diff, base, r.tid, b - m + 1, -1);
                }
                in_run = false;
            }
            if (op == 2u || op == 3u) x += len;
        }
    }
    __syncthreads();
    win_out(W, A.diff, A.asc_off, A.len, t);
}

__global__ __launch_bounds__(kSpanBlock) void pair_scatter_kernel(ScatterArgs A)
{
    // A fragment's closing event lies up to range_max behind its opening one: with inserts of a few hundred bases most of them
    // still fall into the window, and the rest are the plain device atomics the window is there to thin out, not a corner case.
    __shared__ int32_t s_win[kSpanWin];
    __shared__ int32_t s_wpos[kSpanBlock / 64], s_wtid[kSpanBlock / 64];
    __shared__ uint32_t s_aux[kSpanBlock][kAuxWin / 4];
    __shared__ uint32_t s_rg[kRgLds / 4];
    __shared__ int32_t s_generic[2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i = (int64_t)blockIdx.x * kSpanBlock + t;
    win_clear(s_win, t);
    RecView r; r.ok = false; r.flag = 0; r.tid = -1; r.pos = 0; r.mtid = -1; r.mpos = 0; r.isize = 0; r.mapq = 0; r.p = A.recs.raw; r.len = 0; r.o_aux = 0;
    if (i < A.recs.n) r = view_record(A.recs.raw, A.recs.rec_off[i], A.recs.rec_off[i + 1]);
    // what the core decides: about half of the records of a paired library are left mates, and only they walk their tags
    const uint32_t f = r.flag;
    const bool left = r.ok && (f & 0x1u) && !(f & (0x4u | 0x8u | 0x100u | 0x200u | 0x400u | 0x800u)) &&
                      r.tid >= 0 && r.tid < A.n_contigs && r.mtid == r.tid && (((f >> 4) ^ (f >> 5)) & 1u) && r.isize > 0 &&
                      (r.pos < r.mpos || (r.pos == r.mpos && (f & 0x40u))) && (int32_t)r.mapq >= A.min_mapq;
    if (left) {
        // the aux window, as the classify kernel loads it: as many dwords as the record's aux area has
        const uint32_t aux_bytes = r.len - r.o_aux;
#pragma unroll
        for (int k = 0; k < kAuxWin / 4; k++) if (4u * k < aux_bytes) s_aux[t][k] = ld_u32(r.p + r.o_aux + 4u * k);
    }
    // the window starts at the first left mate of the workgroup (nearly all of them are concordant and count)
    win_propose(s_wpos, s_wtid, left, r.pos, r.tid, lane, wave);
    const bool rg_lds = A.rg.bytes <= kRgLds;
    if (rg_lds) for (int k = t; 4 * k < A.rg.bytes; k += kSpanBlock) s_rg[k] = reinterpret_cast<const uint32_t*>(A.rg.blob)[k];
    __syncthreads();
    const SpanWin W = win_open(s_win, s_wpos, s_wtid);
    if (W.tid < 0) return;                                          // no left mate in the whole workgroup
    const RgView T = rg_view(rg_lds ? reinterpret_cast<const uint8_t*>(s_rg) : A.rg.blob, A.rg.n);
    if (t == 0) {
        int32_t rm = 0;
        const bool ok = rg_lookup(T, [](uint32_t k) { return (uint32_t)("generic"[k]); }, 7u, rm);
        s_generic[0] = ok ? 1 : 0; s_generic[1] = rm;
    }
    __syncthreads();

    if (left) {
        AuxWin w; w.lds = s_aux[t]; w.o0 = r.o_aux;
        uint32_t o_rg, o_mq;
        find_rg_mq(r, w, o_rg, o_mq);
        int32_t range_max = s_generic[1];
        const bool known = o_rg ? rg_tag_range(r, w, o_rg, T, range_max) : s_generic[0] != 0;
        if (known && r.isize <= range_max) {
            const int64_t base = A.asc_off[r.tid];
            const int64_t clen = A.len[r.tid], m = A.flank;
            const int64_t a = r.pos < 0 ? 0 : r.pos, e = (int64_t)r.pos + r.isize, b = e > clen ? clen : e;
            if (b - a >= 2 * m) {
                win_event(W, A.diff, base, r.tid, a + m, 1);
                win_event(W, A.diff, base, r.tid, b - m + 1, -1);
            }
        }
    }
    __syncthreads();
    win_out(W, A.diff, A.asc_off, A.len, t);
}

// what the clip scatter takes
struct ClipArgs {
    im_dev_records recs;
    const int64_t* asc_off;
    const int32_t* len;
    int32_t n_contigs;
    int32_t min_clip, min_mapq;
    int32_t* right;             // clipR, genome-wide
    int32_t* left;              // clipL
};

constexpr uint32_t kClipLeftOne = 1u << 16;     // one left clip in a packed window word; a right clip is 1

// Both sides share the window: a word holds the right clips of its position in the low half and the left clips in the high half.
// A workgroup has kSpanBlock = 256 records and a record adds at most one to either half, so no half carries over.
__device__ __forceinline__ void clip_event(const SpanWin& W, int32_t* __restrict__ arr, int64_t base, int32_t tid, int64_t at, bool left)
{
    const int64_t rel = at - W.pos;
    if (tid == W.tid && rel >= 0 && rel < kSpanWin) atomicAdd(reinterpret_cast<uint32_t*>(&W.lds[rel]), left ? kClipLeftOne : 1u);
    else atomicAdd(&arr[base + at], 1);
}

__global__ __launch_bounds__(kSpanBlock) void clip_scatter_kernel(ClipArgs A)
{
    __shared__ int32_t s_win[kSpanWin];
    __shared__ int32_t s_wpos[kSpanBlock / 64], s_wtid[kSpanBlock / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i = (int64_t)blockIdx.x * kSpanBlock + t;
    win_clear(s_win, t);
    SpanRec r; r.ok = false; r.tid = -1; r.pos = 0; r.flag = 0; r.mapq = 0; r.n_cigar = 0; r.o_cigar = 0; r.p = A.recs.raw;
    if (i < A.recs.n) r = span_record(A.recs.raw, A.recs.rec_off[i], A.recs.rec_off[i + 1]);
    const ClipEnds e = clip_decide(r, A.n_contigs, A.min_clip, A.min_mapq);
    const bool clip_l = e.left, clip_r = e.right;
    win_propose(s_wpos, s_wtid, clip_l || clip_r, r.pos, r.tid, lane, wave);
    __syncthreads();
    const SpanWin W = win_open(s_win, s_wpos, s_wtid);
    if (W.tid < 0) return;                                          // no clipped record in the whole workgroup

    if (clip_l || clip_r) {
        int64_t x;
        const bool consumes = clip_refend(r, e, &x);
        if (consumes) {
            const int64_t base = A.asc_off[r.tid], clen = A.len[r.tid];
            if (clip_r && x >= 0 && x <= clen) clip_event(W, A.right, base, r.tid, x, false);
            if (clip_l && r.pos >= 0 && r.pos <= clen) clip_event(W, A.left, base, r.tid, r.pos, true);
        }
    }
    __syncthreads();
    // the gathered window out, unpacked: consecutive lanes hold consecutive positions, only non-zero halves touch memory
    const int64_t at0 = A.asc_off[W.tid] + W.pos;
    const int64_t room = (int64_t)A.len[W.tid] + 1 - W.pos;
#pragma unroll 4
    for (int k = 0; k < kSpanWin / kSpanBlock; k++) {
        const int idx = t + k * kSpanBlock;
        const uint32_t v = (uint32_t)W.lds[idx];
        if (v != 0u && idx < room) {
            if (v & 0xFFFFu) atomicAdd(&A.right[at0 + idx], (int32_t)(v & 0xFFFFu));
            if (v >> 16) atomicAdd(&A.left[at0 + idx], (int32_t)(v >> 16));
        }
    }
}

// for callers that name the events themselves: one lane per event (side 0: clipR, 1: clipL), positions outside [0, clen] dropped
__global__ __launch_bounds__(256) void clip_build_kernel(int32_t n, const int32_t* __restrict__ pos, const uint8_t* __restrict__ side, int64_t clen,
                                                        int32_t* __restrict__ right, int32_t* __restrict__ left)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pos[i];
    if (p < 0 || p > clen) return;
    atomicAdd(side[i] ? &left[p] : &right[p], 1);
}

// One wave per query: the largest count over [beg, end] INCLUSIVE, clipped to [0, clen], of clipR (side 0) or clipL (side 1), and
// the smallest position that holds it; (0, -1) for an interval that is empty after the clip.  Each lane keeps count : ~position as
// one 64-bit key, so the wave's maximum prefers the smaller position among equal counts.  The arrays are counts as they stand:
// no tile sums.
__global__ __launch_bounds__(256) void clip_argmax_kernel(int32_t nq, const uint8_t* __restrict__ side, const int32_t* __restrict__ beg,
                                                         const int32_t* __restrict__ end, const int32_t* __restrict__ right,
                                                         const int32_t* __restrict__ left, int64_t clen,
                                                         uint32_t* __restrict__ count_out, int32_t* __restrict__ pos_out)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < nq; q += nwaves) {
        int64_t a = beg[q], b = end[q];
        if (a < 0) a = 0;
        if (b > clen) b = clen;
        const int32_t* data = side[q] ? left : right;
        uint64_t key = 0;                                           // below every key of a position: ~p > 0 for p < 2^31
        for (int64_t p = a + lane; p <= b; p += 64) {
            const uint64_t k = ((uint64_t)(uint32_t)data[p] << 32) | (0xFFFFFFFFu - (uint32_t)p);
            key = k > key ? k : key;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t hi = (uint32_t)__shfl_xor((int)(key >> 32), o), lo = (uint32_t)__shfl_xor((int)(uint32_t)key, o);
            const uint64_t k = ((uint64_t)hi << 32) | lo;
            key = k > key ? k : key;
        }
        if (lane == 0) {
            count_out[q] = a <= b ? (uint32_t)(key >> 32) : 0u;
            pos_out[q] = a <= b ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
        }
    }
}

// Facing piles (-I): the positions of one contig at which right clips pile up with left clips piling up at or just in front of
// them -- the definition is in include/indelminer_amd.h (seam 5, "Facing piles").  R, L: the contig's clen + 1 counts.
constexpr int kFacingBlock = 256;
constexpr int kFacingPer = 4;                                   // positions of a lane's one 16-byte load
constexpr int kFacingSweeps = 4;                                // loads a lane has in flight: a workgroup owns 4 x 1024 positions
constexpr int kFacingSweep = kFacingBlock * kFacingPer;         // positions a workgroup covers with one load per lane
constexpr int kFacingTile = kFacingSweep * kFacingSweeps;

struct FacingArgs {
    const int32_t* right;
    const int32_t* left;
    int64_t clen;
    int32_t min_reads, max_overlap, cap;
    int32_t* pr;
    int32_t* pl;
    uint32_t* cr;
    uint32_t* cl;
    uint32_t* n_found;
};

// whether p (arr[p] = v) is a PEAK of arr within T: more than every count of [p - T, p), no fewer than every count of (p, p + T],
// the windows stopping at the contig's own entries.  The leftmost of equal peaks wins.  Facing piles test R with it, the peaks
// pass (-U) either array.
__device__ __forceinline__ bool peak_at(const int32_t* __restrict__ arr, int64_t clen, int64_t T, int64_t p, int32_t v)
{
    const int64_t lo = p - T < 0 ? 0 : p - T, hi = p + T > clen ? clen : p + T;
    bool peak = true;
    for (int64_t x = lo; x < p; x++) peak = peak && arr[x] < v;
    for (int64_t x = p + 1; x <= hi; x++) peak = peak && arr[x] <= v;
    return peak;
}

// whether p (R[p] = v >= min_reads) is a peak of R and has a partner in L: the windows stop at the contig's own entries
__device__ __forceinline__ bool facing_at(const FacingArgs& A, int64_t p, int32_t v, int32_t* pl, int32_t* cl)
{
    if (!peak_at(A.right, A.clen, A.max_overlap, p, v)) return false;
    const int64_t lo = p - A.max_overlap < 0 ? 0 : p - A.max_overlap;
    int32_t best = -1;
    int64_t at = p;
    for (int64_t x = p; x >= lo; x--) {                                          // downwards: the largest x among equal counts stays
        const int32_t c = A.left[x];
        if (c > best) { best = c; at = x; }
    }
    *pl = (int32_t)at; *cl = best;
    return best >= A.min_reads;
}

// One streaming pass over one count array (clen + 1 entries), the skeleton of the facing search and of the peaks pass.  A lane
// takes four consecutive positions per 16-byte load, kFacingSweeps loads up front; nearly every lane is done when all of them are
// below m.  The rare lane that is not asks hit(p, c), which reads its windows from memory (L2: the workgroup has just streamed the
// array there).  Hits take their slots with one returning atomic per wave: the rank comes from a ballot, the first lane of the
// ballot adds.  n_found counts every hit; put(slot, p, c) is called only for slots below cap.
template <class Hit, class Put>
__device__ __forceinline__ void clip_stream(const int32_t* __restrict__ arr, int64_t clen, int32_t m, int32_t cap, uint32_t* n_found, Hit hit, Put put)
{
    const int lane = threadIdx.x & 63;
    const int64_t n = clen + 1;
    const int64_t tile = (int64_t)blockIdx.x * kFacingTile;
    int4 v[kFacingSweeps];
#pragma unroll
    for (int s = 0; s < kFacingSweeps; s++) {
        const int64_t p0 = tile + (int64_t)s * kFacingSweep + (int64_t)threadIdx.x * kFacingPer;
        if (p0 + kFacingPer <= n) v[s] = *reinterpret_cast<const int4*>(arr + p0);
        else {
            // the contig's last entries: one by one, nothing is read behind entry clen
            v[s].x = p0 < n ? arr[p0] : 0; v[s].y = p0 + 1 < n ? arr[p0 + 1] : 0;
            v[s].z = p0 + 2 < n ? arr[p0 + 2] : 0; v[s].w = 0;
        }
    }
#pragma unroll
    for (int s = 0; s < kFacingSweeps; s++) {
        const bool any = v[s].x >= m || v[s].y >= m || v[s].z >= m || v[s].w >= m;
        if (!__ballot(any)) continue;                                            // wave-uniform: almost every sweep of every wave
        const int64_t p0 = tile + (int64_t)s * kFacingSweep + (int64_t)threadIdx.x * kFacingPer;
#pragma unroll
        for (int j = 0; j < kFacingPer; j++) {
            const int32_t c = j == 0 ? v[s].x : j == 1 ? v[s].y : j == 2 ? v[s].z : v[s].w;
            const int64_t p = p0 + j;
            const bool pile = c >= m && p < n && hit(p, c);
            const uint64_t piles = __ballot(pile);
            if (!piles) continue;
            const int first = (int)__builtin_ctzll(piles);
            uint32_t base = 0;
            if (lane == first) base = atomicAdd(n_found, (uint32_t)__builtin_popcountll(piles));
            base = (uint32_t)__shfl((int)base, first);
            const uint32_t slot = base + (uint32_t)__builtin_popcountll(piles & ((1ull << lane) - 1ull));
            if (pile && slot < (uint32_t)cap) put(slot, p, c);
        }
    }
}

// The facing search: the stream runs over R, L is read only by the lane that holds a peak.
__global__ __launch_bounds__(kFacingBlock) void clip_facing_kernel(FacingArgs A)
{
    int32_t pl = 0, cl = 0;
    clip_stream(A.right, A.clen, A.min_reads, A.cap, A.n_found,
                [&](int64_t p, int32_t c) { return facing_at(A, p, c, &pl, &cl); },
                [&](uint32_t slot, int64_t p, int32_t c) { A.pr[slot] = (int32_t)p; A.pl[slot] = pl; A.cr[slot] = (uint32_t)c; A.cl[slot] = (uint32_t)cl; });
}

struct PeaksArgs {
    const int32_t* arr;
    int64_t clen;
    int32_t min_reads, reach, cap;
    int32_t* pos;
    uint32_t* count;
    uint32_t* n_found;
};

// The peaks of ONE array (-U; include/indelminer_amd.h, seam 5, "Crossed piles"): the same stream, the peak test alone.  It runs once
// per side.
__global__ __launch_bounds__(kFacingBlock) void clip_peaks_kernel(PeaksArgs A)
{
    clip_stream(A.arr, A.clen, A.min_reads, A.cap, A.n_found,
                [&](int64_t p, int32_t c) { return peak_at(A.arr, A.clen, A.reach, p, c); },
                [&](uint32_t slot, int64_t p, int32_t c) { A.pos[slot] = (int32_t)p; A.count[slot] = (uint32_t)c; });
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

// One LANE per end (-K): the minimum of span[p] of contig tid[k] over [pos[k] - slack, pos[k] + slack], clipped to [0, len[tid[k]]]:
// what span_query_kernel answers for that interval of that contig.  The ends of a call lie on any contigs, so every lane finds its own
// contig's run in the genome-wide array through asc_off (the scatter's 64-bit offsets) and its contig's run of tile offsets through
// sums_off[k], which the entry point names per end.  The driver asks with slack 0: one load of the array and one of the offsets per
// lane, no cross-lane operation, nothing divergent to wait for.  The loop has 2 slack + 1 <= 511 turns for any input.  An end whose
// contig is not one of the reference's answers 0 and reads nothing (the entry point has refused it before).
constexpr int kEndsBlock = 256;

__global__ __launch_bounds__(kEndsBlock) void span_ends_kernel(SpanEndsArgs A)
{
    const int64_t k = (int64_t)blockIdx.x * kEndsBlock + threadIdx.x;
    if (k >= A.n) return;
    const int32_t t = A.tid[k];
    if (t < 0 || t >= A.n_contigs) { A.out[k] = 0u; return; }
    const int64_t clen = A.len[t], lo = (int64_t)A.pos[k] - A.slack;
    const int32_t* __restrict__ data = A.span + A.asc_off[t];
    const int32_t* __restrict__ offs = A.sums + A.sums_off[k];
    uint32_t mn = 0xFFFFFFFFu;
    bool any = false;
    for (int32_t j = 0; j <= 2 * A.slack; j++) {
        const int64_t p = lo + j;
        if (p < 0 || p > clen) continue;
        mn = min(mn, (uint32_t)(data[p] + offs[p / kScanTile]));
        any = true;
    }
    A.out[k] = any ? mn : 0u;
}

hipError_t launch_scatter(void (*kernel)(ScatterArgs), const RefDev& ref, const RgTable& rg, int32_t flank, int32_t min_mapq, const im_dev_records& recs,
                          int32_t* diff, hipStream_t stream)
{
    if (recs.n <= 0) return hipSuccess;
    ScatterArgs A;
    A.recs = recs; A.asc_off = ref.asc_off; A.len = ref.len; A.n_contigs = ref.n_contigs;
    A.flank = flank; A.min_mapq = min_mapq; A.rg = rg; A.diff = diff;
    const int blocks = (recs.n + kSpanBlock - 1) / kSpanBlock;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kSpanBlock), 0, stream, A);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_span_scatter(const RefDev& ref, int32_t flank, int32_t min_mapq, const im_dev_records& recs, int32_t* diff, hipStream_t stream)
{
    return launch_scatter(span_scatter_kernel, ref, RgTable{nullptr, 0, 0}, flank, min_mapq, recs, diff, stream);
}

hipError_t launch_pair_scatter(const RefDev& ref, const RgTable& rg, int32_t flank, int32_t min_mapq, const im_dev_records& recs, int32_t* diff, hipStream_t stream)
{
    return launch_scatter(pair_scatter_kernel, ref, rg, flank, min_mapq, recs, diff, stream);
}

hipError_t launch_clip_scatter(const RefDev& ref, int32_t min_clip, int32_t min_mapq, const im_dev_records& recs, int32_t* right, int32_t* left,
                               hipStream_t stream)
{
    if (recs.n <= 0) return hipSuccess;
    ClipArgs A;
    A.recs = recs; A.asc_off = ref.asc_off; A.len = ref.len; A.n_contigs = ref.n_contigs;
    A.min_clip = min_clip; A.min_mapq = min_mapq; A.right = right; A.left = left;
    const int blocks = (recs.n + kSpanBlock - 1) / kSpanBlock;
    hipLaunchKernelGGL(clip_scatter_kernel, dim3(blocks), dim3(kSpanBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_clip_build(int64_t clen, int32_t n, const int32_t* pos, const uint8_t* side, int32_t* right, int32_t* left, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(right, 0, (size_t)(clen + 1) * sizeof(int32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(left, 0, (size_t)(clen + 1) * sizeof(int32_t), stream);
    if (e != hipSuccess || n <= 0) return e;
    hipLaunchKernelGGL(clip_build_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, pos, side, clen, right, left);
    return hipGetLastError();
}

hipError_t launch_clip_argmax(int32_t nq, const uint8_t* side, const int32_t* beg, const int32_t* end, const int32_t* right, const int32_t* left,
                              int64_t clen, uint32_t* count_out, int32_t* pos_out, hipStream_t stream)
{
    if (nq <= 0) return hipSuccess;
    int b = (nq + 3) / 4;
    if (b > 2048) b = 2048;
    hipLaunchKernelGGL(clip_argmax_kernel, dim3(b), dim3(256), 0, stream, nq, side, beg, end, right, left, clen, count_out, pos_out);
    return hipGetLastError();
}

hipError_t launch_clip_facing(const int32_t* right, const int32_t* left, int64_t clen, int32_t min_reads, int32_t max_overlap, int32_t cap,
                              int32_t* pr, int32_t* pl, uint32_t* cr, uint32_t* cl, uint32_t* n_found, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(n_found, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    FacingArgs A;
    A.right = right; A.left = left; A.clen = clen; A.min_reads = min_reads; A.max_overlap = max_overlap; A.cap = cap;
    A.pr = pr; A.pl = pl; A.cr = cr; A.cl = cl; A.n_found = n_found;
    const int64_t blocks = (clen + 1 + kFacingTile - 1) / kFacingTile;          // clen <= 0x7fffff00: at most 2^19 workgroups
    hipLaunchKernelGGL(clip_facing_kernel, dim3((unsigned)blocks), dim3(kFacingBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_clip_peaks(const int32_t* arr, int64_t clen, int32_t min_reads, int32_t reach, int32_t cap, int32_t* pos, uint32_t* count,
                             uint32_t* n_found, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(n_found, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    PeaksArgs A;
    A.arr = arr; A.clen = clen; A.min_reads = min_reads; A.reach = reach; A.cap = cap; A.pos = pos; A.count = count; A.n_found = n_found;
    const int64_t blocks = (clen + 1 + kFacingTile - 1) / kFacingTile;
    hipLaunchKernelGGL(clip_peaks_kernel, dim3((unsigned)blocks), dim3(kFacingBlock), 0, stream, A);
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

hipError_t launch_span_query_ends(const SpanEndsArgs& A, hipStream_t stream)
{
    if (A.n <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((int64_t)A.n + kEndsBlock - 1) / kEndsBlock);
    hipLaunchKernelGGL(span_ends_kernel, dim3(blocks), dim3(kEndsBlock), 0, stream, A);
    return hipGetLastError();
}

}  // namespace im
