// im_links.hip -- the three families of links kept in keyed tables of their own (gfx950): two of read pairs, one of split reads:
//   the PAIR LINKS (-M): the read pairs whose orientation says "junction", counted between two windows.  The definition is in
//     include/indelminer_amd.h (seam 5, "Pair links"); DESIGN.md 4.5j has the cost.
//   the MATE LINKS (-T): the read pairs whose mate lies on ANOTHER contig, asked where the mates of the reads around a position lie.
//     The definition is in include/indelminer_amd.h (seam 5, "Mate links"); DESIGN.md 4.5k has the cost.
//   the SPLIT LINKS (-S): the primary records whose SA:Z tag places their clipped part elsewhere, counted between two junction ends.
//     The definition is in include/indelminer_amd.h (seam 5, "Split links"); DESIGN.md 4.5l has the rest.
//
// PAIR LINKS  A delivered record that is the leftmost of a pair on one contig, both reads mapped, neither read in the normal orientation
// (forward in front of reverse), stores ONE LINK (tid, kind, pos, mpos): kind 0 EVERTED (this read reverse, its mate forward: a tandem
// duplication's pairs), 1 FORWARD (both forward: an inversion's left junction), 2 REVERSE (both reverse: its right junction).
//
// MATE LINKS  A delivered record that is paired, both reads mapped, its mate on another contig, stores ONE LINK (tid, kind, pos, mtid,
// mpos) at its own contig: kind = r | m << 1, r = this read reverse, m = its mate reverse.  Both reads of a pair store one each.
//
// SPLIT LINKS  A delivered primary record with a qualifying soft clip whose SA:Z tag holds exactly one entry stores ONE LINK
// (tidA, pA, sideA, tidB, pB, sideB): end A is the clip's (-C's position and side), end B where the entry's alignment continues;
// kind = sideA | sideB << 1.  The front of its rule differs from the pairs' (paired or not does not matter) and it reads the CIGAR
// and the aux area, so it has a scatter kernel of its own; the key, the tickets, the insert and the bucket walk are the shared ones.
//
// THE TABLES are keyed tables of im_keyed.hpp (slots, tickets, claim, walk), an allocation each, with
//   word 0   the key, EVERY FAMILY'S: bit 63 set (an empty slot is 0) | tid << 26 | (pos >> 8) << 2 | kind   (tid < 2^24, pos < 2^31)
//   word 1   the payload, the family's own:   pair links  pos | mpos << 32        mate links  pos & 255 | mtid << 8 | mpos << 32
//                                                       split links  pA & 255 | tidB << 8 | pB << 32   (the key: tidA, pA >> 8)
// The whole key enters the hash: every link of one (tid, 256-base bucket, kind) lies on one probe run.
//
// SHARED: the key, the bucket, the block sizes, the scatter (link_scatter<Rule>: the front of the record rule, the tickets, the insert)
// and the interval and the bucket loop of the queries (link_clip, link_walk).  PER FAMILY: the payload, the rest of the record rule, the add kernel's range checks
// and what a query does with the links it is handed.
//
//   pairlink_scatter, matelink_scatter   one lane per delivered record; the lanes that hold a link insert it, on tickets their
//                                        workgroup draws with one atomic add
//   pairlink_add, matelink_add           one lane per link, for callers that name the events themselves
//   pairlink_count     one wave per query (kind, a0, a1, b0, b1): the links with pos in [a0, a1], mpos in [b0, b1], mpos - pos >= min_sep
//   matelink_partner   one wave per query (kind, a0, a1): the links with pos in [a0, a1] vote for the cell (mtid, mpos >> 10) of their
//                      mate in a table in LDS; the pair of neighbouring cells with the most links wins
//   splitlink_scatter  one lane per delivered record: front, CIGAR ends, then -- the few lanes with a qualifying clip -- the walk to
//                      SA:Z (find_tag, im_rg.hpp), the parse of its one entry and the contig-name look-up; tickets as above
//   splitlink_add      one lane per link the caller names, as six columns
//   splitlink_count    one wave per query (tid1, side1, [a0, a1], tid2, side2, [b0, b1]): the links between the two ends
//
// THE SPLIT JUNCTIONS (-J): the junctions the stored split links name by themselves, searched in the table alone.  The rule is in
// include/indelminer_amd.h (seam 5, "Split junctions"); DESIGN.md 4.5m has the rest.  Three launches of one call, made once per run:
//   splitjunc_sweep    one lane per slot: the occupied slots into a list, on ranks the workgroup draws with one atomic add
//   splitjunc_count    one wave per listed link: E, the two window counts and the one emitter among equal links
//   splitjunc_peak     one wave per 64 listed links: an emitter's neighbours' E decide the peak; rows through one ballot and one atomic add
//
// THE JUNCTION OVERLAP (-H): the read bases the two parts of a split read share, or that lie between them, as a 16-bit code per SLOT in
// an array beside the split-link table.  The rule is in include/indelminer_amd.h (seam 5, "Junction overlap"); DESIGN.md 4.5o has the rest.
//   splitlink_scatter_overlap, splitlink_add_overlap   the scatter and the add, which also leave the link's code at the slot it claimed
//                                                      (keyed_place_at); the links stored and the tickets are those of the forms without
//   splitlink_overlap  one wave per junction: the known codes of the links between its two windows, from either end -- their number,
//                      their lower median by bisection over the code (18 walks of the same probe runs, no memory), and how many equal it
//
// THE JUNCTION PAIRS (-E): the read pairs on either side of a junction, out of the two pair tables.  The rule is in
// include/indelminer_amd.h (seam 5, "Junction pairs"); DESIGN.md 4.5p has the rest.
//   pairlink_scatter_stretched   the pair links' scatter with a fourth kind, 3 STRETCHED: the normal orientation that the aligner has
//                                NOT flagged a proper pair (a deletion's pairs); the links of kinds 0 .. 2 are those of the form without
//   junction_pairs     one wave per junction, ends on any contigs: one contig -- the pair links of the kind the two sides name between
//                      the two windows; two contigs -- the mate links from either end's window into the other's

#include "im_keyed.hpp"
#include "im_rg.hpp"
#include "im_wave.hpp"

namespace im {
namespace {

constexpr int kLinkBlock = 1024;      // records of a scatter workgroup: one ticket draw each
constexpr int kLinkWaveBlock = 256;   // threads of the add and query kernels
constexpr int kLinkBucketShift = 8;   // a bucket is 256 bases: a query window of 1 000 bases walks 4 or 5 probe runs
constexpr int kMateCellShift = 10;    // a cell is 1 024 bases of the mate's contig
constexpr int kMateCells = IM_MATELINK_CELLS;
static_assert(kMateCells == 256, "a cell's slot is the top 8 bits of its hash, and a lane owns kMateCells / 64 slots");

__device__ __forceinline__ uint64_t link_key(int32_t tid, int64_t bucket, uint32_t kind)
{
    return kKeyedUsed | ((uint64_t)(uint32_t)tid << 26) | ((uint64_t)bucket << 2) | kind;
}

__device__ __forceinline__ uint64_t pair_payload(int64_t pos, int64_t mpos) { return (uint64_t)(uint32_t)pos | ((uint64_t)(uint32_t)mpos << 32); }

__device__ __forceinline__ uint64_t mate_payload(int64_t pos, int32_t mtid, int64_t mpos)
{
    return (uint64_t)((uint32_t)pos & 255u) | ((uint64_t)(uint32_t)mtid << 8) | ((uint64_t)(uint32_t)mpos << 32);
}

struct LinkScatterArgs {
    im_dev_records recs;
    const int32_t* len;
    int32_t n_contigs, min_mapq;
    KeyedTable tab;
};

// The record rules, on the 32-byte core alone.  A rule says whether a record that has passed the front both share (link_of_record)
// stores a link; *kind, *payload: what it stores, under the key of (r.tid, r.pos's bucket, *kind).  The front has held r.tid to
// [0, n_contigs): len[r.tid] may be read; len[r.mtid] only behind the rule's own check of r.mtid.
//
// kStretched (-E; include/indelminer_amd.h, "Junction pairs"): the normal orientation is a link of kind 3 when the aligner has not
// flagged the pair proper (0x2 clear).  The links of kinds 0 .. 2 are the same in either form; the form without is the rule as it was.
template <bool kStretched>
struct PairRule {
    static __device__ __forceinline__ bool link(const LinkScatterArgs& A, const RecView& r, uint32_t* kind, uint64_t* payload)
    {
        if (r.mtid != r.tid) return false;
        if (!(r.pos < r.mpos || (r.pos == r.mpos && (r.flag & 0x40u)))) return false;      // each pair once, at its leftmost record
        const uint32_t rev = (r.flag >> 4) & 1u, mrev = (r.flag >> 5) & 1u;
        if constexpr (kStretched) {
            if (!rev && mrev && (r.flag & 0x2u)) return false;          // a proper pair is no link: the aligner's verdict on its insert size
        } else {
            if (!rev && mrev) return false;                             // the normal orientation is no link, whatever its insert size
        }
        if (r.pos < 0 || r.mpos > A.len[r.tid]) return false;          // pos <= mpos behind the leftmost test: both lie in [0, len[tid]]
        if constexpr (kStretched) *kind = rev ? (mrev ? 2u : 0u) : (mrev ? 3u : 1u);
        else *kind = rev ? (mrev ? 2u : 0u) : 1u;
        *payload = pair_payload(r.pos, r.mpos);
        return true;
    }
};

struct MateRule {
    static __device__ __forceinline__ bool link(const LinkScatterArgs& A, const RecView& r, uint32_t* kind, uint64_t* payload)
    {
        if (r.mtid < 0 || r.mtid >= A.n_contigs || r.mtid == r.tid) return false;
        if (r.pos < 0 || r.pos > A.len[r.tid] || r.mpos < 0 || r.mpos > A.len[r.mtid]) return false;
        *kind = ((r.flag >> 4) & 1u) | (((r.flag >> 5) & 1u) << 1);
        *payload = mate_payload(r.pos, r.mtid, r.mpos);
        return true;
    }
};

// Whether record i stores a link; *key, *payload: what it stores.  The front of both rules: a whole core, paired, this read and its
// mate mapped, primary, no duplicate, no failure, on a contig of the reference, at min_mapq or above.
template <class Rule>
__device__ __forceinline__ bool link_of_record(const LinkScatterArgs& A, int64_t i, uint64_t* key, uint64_t* payload)
{
    if (i >= A.recs.n) return false;
    const RecView r = view_record(A.recs.raw, A.recs.rec_off[i], A.recs.rec_off[i + 1]);
    if (r.len < 32u) return false;
    if ((int32_t)r.mapq < A.min_mapq) return false;
    if (!(r.flag & 0x1u) || (r.flag & (0x4u | 0x8u | 0x100u | 0x200u | 0x400u | 0x800u))) return false;
    if (r.tid < 0 || r.tid >= A.n_contigs) return false;
    uint32_t kind;
    if (!Rule::link(A, r, &kind, payload)) return false;
    *key = link_key(r.tid, r.pos >> kLinkBucketShift, kind);
    return true;
}

// One lane per record; one ticket draw per workgroup (keyed_block_tickets has the reason); a workgroup without a link -- most of
// them -- ends there.
template <class Rule>
__device__ __forceinline__ void link_scatter(const LinkScatterArgs& A)
{
    uint64_t key = 0, payload = 0;
    const bool has = link_of_record<Rule>(A, (int64_t)blockIdx.x * kLinkBlock + threadIdx.x, &key, &payload);
    unsigned long long ticket;
    if (!keyed_block_tickets<kLinkBlock, 1>(A.tab, has ? 1u : 0u, &ticket)) return;
    if (has && keyed_admit(A.tab, ticket)) keyed_place(A.tab, keyed_home(key, A.tab.log2_slots), key, payload);
}

__global__ __launch_bounds__(kLinkBlock) void pairlink_scatter_kernel(LinkScatterArgs A) { link_scatter<PairRule<false>>(A); }
__global__ __launch_bounds__(kLinkBlock) void pairlink_scatter_stretched_kernel(LinkScatterArgs A) { link_scatter<PairRule<true>>(A); }
__global__ __launch_bounds__(kLinkBlock) void matelink_scatter_kernel(LinkScatterArgs A) { link_scatter<MateRule>(A); }

// for callers that name the events themselves: one lane per link; positions outside [0, clen] are dropped (no ticket)
__global__ __launch_bounds__(kLinkWaveBlock) void pairlink_add_kernel(int32_t n, int32_t tid, int64_t clen, const int32_t* __restrict__ pos,
                                                                      const int32_t* __restrict__ mpos, const uint8_t* __restrict__ kind, KeyedTable tab)
{
    const int64_t i = (int64_t)blockIdx.x * kLinkWaveBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pos[i], m = mpos[i];
    if (p < 0 || p > clen || m < 0 || m > clen) return;
    const uint64_t key = link_key(tid, p >> kLinkBucketShift, kind[i]);
    keyed_insert(tab, keyed_home(key, tab.log2_slots), key, pair_payload(p, m));
}

// the same for the mate links; a link that fails the rule's range checks is dropped (no ticket)
__global__ __launch_bounds__(kLinkWaveBlock) void matelink_add_kernel(int32_t n, int32_t tid, const int32_t* __restrict__ len, int32_t n_contigs,
                                                                      const int32_t* __restrict__ pos, const int32_t* __restrict__ mtid,
                                                                      const int32_t* __restrict__ mpos, const uint8_t* __restrict__ kind, KeyedTable tab)
{
    const int64_t i = (int64_t)blockIdx.x * kLinkWaveBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pos[i], m = mpos[i];
    const int32_t mt = mtid[i];
    if (mt < 0 || mt >= n_contigs || mt == tid) return;
    if (p < 0 || p > len[tid] || m < 0 || m > len[mt]) return;
    const uint64_t key = link_key(tid, p >> kLinkBucketShift, kind[i]);
    keyed_insert(tab, keyed_home(key, tab.log2_slots), key, mate_payload(p, mt, m));
}

// What both queries do with an interval, by the whole wave.  link_clip: [*lo, *hi] clipped to [0, clen], in place; whether anything is
// left of it.  link_walk, for a pos interval that link_clip has left something of: for every bucket of it (at most 257: the caller
// holds a1 - a0 to 65 535) the wave walks the bucket's probe run (keyed_walk) for the slots whose key is the bucket's, and
// each(has, bucket, payload) is called for every batch that holds one: has says whether this lane's slot does, and payload is that
// slot's (0 without).  Every branch is on values the whole wave shares; both loops are bounded, by the bucket count and the slot count.
__device__ __forceinline__ bool link_clip(int64_t* lo, int64_t* hi, int64_t clen)
{
    *lo = *lo < 0 ? 0 : *lo;
    *hi = *hi > clen ? clen : *hi;
    return *lo <= *hi;
}

template <class Each>
__device__ __forceinline__ void link_walk(const KeyedTable& T, int32_t tid, uint32_t kind, int64_t a0, int64_t a1, int lane, Each each)
{
    for (int64_t bucket = a0 >> kLinkBucketShift; bucket <= (a1 >> kLinkBucketShift); bucket++) {
        const uint64_t want = link_key(tid, bucket, kind);
        (void)keyed_walk(T, keyed_home(want, T.log2_slots), [want](uint64_t key) { return key == want; }, lane,
                         [&](bool has, uint64_t, uint64_t s) { each(has, bucket, has ? T.slots[2ull * s + 1ull] : 0ull); });
    }
}

struct LinkCountArgs {
    int32_t nq, tid, min_sep;
    const uint8_t* kind;
    const int32_t* a0;
    const int32_t* a1;
    const int32_t* b0;
    const int32_t* b1;
    int64_t clen;
    KeyedTable tab;
    uint32_t* count;
};

// One wave per query.  Both intervals are clipped to [0, clen].  A lane's link counts when its payload passes the three tests; the wave
// sums by ballot and popcount.
__global__ __launch_bounds__(kLinkWaveBlock) void pairlink_count_kernel(LinkCountArgs A)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < A.nq; q += nwaves) {
        int64_t a0 = A.a0[q], a1 = A.a1[q], b0 = A.b0[q], b1 = A.b1[q];
        const uint32_t kind = A.kind[q];
        const bool in_a = link_clip(&a0, &a1, A.clen), in_b = link_clip(&b0, &b1, A.clen);
        uint32_t n = 0;
        if (in_a && in_b) {
            link_walk(A.tab, A.tid, kind, a0, a1, lane, [&](bool has, int64_t, uint64_t payload) {
                const int64_t pos = (int64_t)(uint32_t)payload, mpos = (int64_t)(uint32_t)(payload >> 32);
                const bool counts = has && pos >= a0 && pos <= a1 && mpos >= b0 && mpos <= b1 && mpos - pos >= (int64_t)A.min_sep;
                n += (uint32_t)__builtin_popcountll(__ballot(counts));
            });
        }
        if (lane == 0) A.count[q] = n;
    }
}

// The cells of one query, one table per wave: open addressing over kMateCells slots of 20 bytes, ALL of which may be taken -- a 257th
// distinct cell finds no slot on its way round, and that is the cap of the definition.
//   key   bit 63 set (an empty slot is 0) | mtid << 32 | mpos >> 10: the right neighbour of a cell is key + 1 (mpos >> 10 < 2^21)
struct MateCellTable {
    unsigned long long key[kMateCells];
    uint32_t cnt[kMateCells], lo[kMateCells], hi[kMateCells];
};
static_assert(sizeof(MateCellTable) == 20 * kMateCells, "20 bytes a cell: 5 KB per wave");

__device__ __forceinline__ uint32_t cell_home(unsigned long long cell) { return (uint32_t)((cell * kKeyedHashMul) >> 56); }

// The slot that holds `cell`, or kMateCells when the table does not: the lanes with want set probe from the cell's home until they see
// the cell or an empty slot; the loop is the wave's, bounded by the slot count.
__device__ __forceinline__ uint32_t cell_find(const MateCellTable& C, unsigned long long cell, bool want)
{
    uint32_t s = cell_home(cell), found = (uint32_t)kMateCells;
    for (int step = 0; step < kMateCells; step++) {
        if (!__ballot(want)) break;                                 // wave-uniform
        if (want) {
            const unsigned long long k = C.key[s];
            if (k == cell) { found = s; want = false; }
            else if (k == 0ull) want = false;
            else s = (s + 1u) & (uint32_t)(kMateCells - 1);
        }
    }
    return found;
}

struct MatePartnerArgs {
    int32_t nq, tid;
    const uint8_t* kind;
    const int32_t* a0;
    const int32_t* a1;
    int64_t clen;
    KeyedTable tab;
    uint32_t* n_links;
    int32_t* mtid;
    uint32_t* n_partner;
    int32_t* lo;
    int32_t* hi;
};

// One wave per query.  A lane whose slot holds a link of the interval (link_walk) claims the link's cell in the wave's LDS table with a
// 64-bit compare-and-swap and adds the link to the cell's count, minimum and maximum with LDS atomics: sums, minima and maxima, so
// nothing depends on the order of arrival, and a cell finds no slot only when 256 others hold them all.  Then every lane takes four
// slots: an occupied one looks up its right neighbour, its score is the two counts, and the wave reduces (score, the smallest cell key
// among equals -- mtid in the high word, the cell in the low one).  A cell (mtid, c) that holds no link while (mtid, c + 1) does need
// not stand: its links are those of (mtid, c + 1) or fewer, and the answer names links, not c.  Every branch is on values the whole
// wave shares; every loop is bounded, by the bucket count, the slot count or kMateCells.  The LDS one lane writes and another reads is
// ordered by wave_lds_sync (im_wave.hpp): LDS executes a wave's instructions in order.
__global__ __launch_bounds__(kLinkWaveBlock) void matelink_partner_kernel(MatePartnerArgs A)
{
    __shared__ MateCellTable s_cells[kLinkWaveBlock / 64];
    const int lane = threadIdx.x & 63;
    MateCellTable& C = s_cells[threadIdx.x >> 6];
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < A.nq; q += nwaves) {
        int64_t a0 = A.a0[q], a1 = A.a1[q];
        const uint32_t kind = A.kind[q];
        const bool any = link_clip(&a0, &a1, A.clen);
#pragma unroll
        for (int j = 0; j < kMateCells / 64; j++) {
            const int s = lane + 64 * j;
            C.key[s] = 0ull; C.cnt[s] = 0u; C.lo[s] = 0xFFFFFFFFu; C.hi[s] = 0u;
        }
        wave_lds_sync();
        uint32_t n = 0;
        bool over = false;
        if (any) link_walk(A.tab, A.tid, kind, a0, a1, lane, [&](bool has, int64_t bucket, uint64_t payload) {
            const int64_t pos = (bucket << kLinkBucketShift) | (int64_t)(payload & 255ull);
            bool pending = has && pos >= a0 && pos <= a1;
            n += (uint32_t)__builtin_popcountll(__ballot(pending));
            const uint32_t mpos = (uint32_t)(payload >> 32);
            const unsigned long long cell = kKeyedUsed | ((unsigned long long)(((uint32_t)payload >> 8) & 0xFFFFFFu) << 32) | (mpos >> kMateCellShift);
            uint32_t c = cell_home(cell);
            for (int step = 0; step < kMateCells; step++) {
                if (!__ballot(pending)) break;              // wave-uniform
                if (pending) {
                    const unsigned long long prev = atomicCAS(&C.key[c], 0ull, cell);
                    if (prev == 0ull || prev == cell) {
                        atomicAdd(&C.cnt[c], 1u); atomicMin(&C.lo[c], mpos); atomicMax(&C.hi[c], mpos);
                        pending = false;
                    } else {
                        c = (c + 1u) & (uint32_t)(kMateCells - 1);
                    }
                }
            }
            over = over || __ballot(pending) != 0ull;
        });
        wave_lds_sync();
        // this lane's best of its four slots: the larger score, the smaller cell key among equals
        uint32_t best_score = 0;
        unsigned long long best_cell = ~0ull;
#pragma unroll
        for (int j = 0; j < kMateCells / 64; j++) {
            const int s = lane + 64 * j;
            const unsigned long long cell = C.key[s];
            const uint32_t right = cell_find(C, cell + 1ull, cell != 0ull);
            const uint32_t score = cell != 0ull ? C.cnt[s] + (right < (uint32_t)kMateCells ? C.cnt[right] : 0u) : 0u;
            if (score > best_score || (score == best_score && score != 0u && cell < best_cell)) { best_score = score; best_cell = cell; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t sc = (uint32_t)__shfl_xor((int)best_score, o);
            const uint32_t chi = (uint32_t)__shfl_xor((int)(uint32_t)(best_cell >> 32), o), clo = (uint32_t)__shfl_xor((int)(uint32_t)best_cell, o);
            const unsigned long long cell = ((unsigned long long)chi << 32) | clo;
            if (sc > best_score || (sc == best_score && cell < best_cell)) { best_score = sc; best_cell = cell; }
        }
        // the winner's links: its own cell and the right neighbour, looked up by the whole wave (one address: a broadcast)
        int32_t mtid = -1, lo = 0, hi = 0;
        uint32_t n_partner = 0;
        if (over) {
            mtid = -2;
        } else if (best_score != 0u) {                              // wave-uniform
            const uint32_t own = cell_find(C, best_cell, true), right = cell_find(C, best_cell + 1ull, true);
            uint32_t l = 0xFFFFFFFFu, h = 0u;
            if (own < (uint32_t)kMateCells) { l = C.lo[own]; h = C.hi[own]; }
            if (right < (uint32_t)kMateCells) { l = l < C.lo[right] ? l : C.lo[right]; h = h > C.hi[right] ? h : C.hi[right]; }
            mtid = (int32_t)((uint32_t)(best_cell >> 32) & 0xFFFFFFu); n_partner = best_score; lo = (int32_t)l; hi = (int32_t)h;
        }
        if (lane == 0) { A.n_links[q] = n; A.mtid[q] = mtid; A.n_partner[q] = n_partner; A.lo[q] = lo; A.hi[q] = hi; }
        wave_lds_sync();                                            // the next query clears what this one has read
    }
}

// ---- the split links (-S) ----------

__device__ __forceinline__ uint64_t split_payload(int64_t pa, int32_t tidb, int64_t pb)
{
    return (uint64_t)((uint32_t)pa & 255u) | ((uint64_t)(uint32_t)tidb << 8) | ((uint64_t)(uint32_t)pb << 32);
}

// The contig names as one blob, the layout idea of RgView (im_rg.hpp), built by im_splitlink_enable:
//   int32 [0] bins (a power of two)  [1] n   [2 .. 2 + bins] bin_start   then tid[n], name_off[n], name_len[n] in bin order, then the names
// The bin of a name is its 32-bit FNV-1a hash & (bins - 1).  The compare is exact, over the whole length: ctg1 is not ctg10.
__device__ __forceinline__ uint32_t name_hash_step(uint32_t h, uint32_t byte) { return (h ^ byte) * 16777619u; }
constexpr uint32_t kNameHashSeed = 2166136261u;

__device__ __forceinline__ int32_t contig_of_name(const uint8_t* blob, const uint8_t* name, uint32_t len, uint32_t hash)
{
    const int32_t* w = reinterpret_cast<const int32_t*>(blob);
    const int32_t bins = w[0], n = w[1];
    const int32_t* bin_start = w + 2;
    const int32_t* e_tid = bin_start + bins + 1;
    const int32_t* e_off = e_tid + n;
    const int32_t* e_len = e_off + n;
    const uint8_t* names = reinterpret_cast<const uint8_t*>(e_len + n);
    const uint32_t bin = hash & (uint32_t)(bins - 1);
    for (int32_t e = bin_start[bin]; e < bin_start[bin + 1]; e++) {
        if ((uint32_t)e_len[e] != len) continue;
        const uint8_t* en = names + e_off[e];
        bool same = true;
        for (uint32_t i = 0; i < len && same; i++) same = en[i] == name[i];
        if (same) return e_tid[e];
    }
    return -1;
}

// What the one entry of an SA:Z value says (include/indelminer_amd.h, "Split links", the table of fields)
struct SaEntry {
    uint32_t o_name, name_len, name_hash;
    int64_t pos;            // 1-based, 1 .. 2^31 - 1
    int64_t span;           // its M = X D N lengths
    int64_t qlen;           // Q2 of "Junction overlap": its M I S H = X lengths
    uint32_t lead, trail;   // its first / last operation's length when that is S or H, else 0
    uint32_t mapq;
    bool minus;
};

// The value from offset o on, a byte per pass: the loop is the WAVE's, the lanes that are done (or never parse: `on` false)
// predicated; a pass ends at the record's end at the latest (o < r.len wherever a byte is read or the window moved).  true iff the
// value is exactly one well-formed entry followed by ';' NUL or by NUL.
__device__ __forceinline__ bool parse_sa(const RecView& r, AuxWin& w, uint32_t o, bool on, SaEntry* e)
{
    e->o_name = o; e->name_len = 0; e->name_hash = kNameHashSeed; e->pos = 0; e->span = 0; e->qlen = 0; e->lead = e->trail = 0; e->mapq = 0; e->minus = false;
    // st: 0 rname, 1 pos, 2 strand, 3 the comma behind it, 4 cigar, 5 mapQ, 6 NM, 7 behind ';'
    uint32_t st = 0, nd = 0, nops = 0;
    uint64_t val = 0;
    bool ok = false;
    for (;;) {
        on = on && o < r.len;
        if (__ballot(on) == 0ull) break;
        const bool mv = on && o - w.o0 >= (uint32_t)kAuxWin;
        if (__ballot(mv) != 0ull) { if (mv) aux_slide(r, w, o); }
        if (on) {
            const uint32_t b = win_byte(w, o, true), d = b - (uint32_t)'0';
            const bool dig = d < 10u;
            o++;
            if (st == 0u) {
                if (b == ',') { on = e->name_len >= 1u; st = 1u; }
                else if (b == ';' || b == 0u) on = false;
                else { e->name_hash = name_hash_step(e->name_hash, b); e->name_len++; }
            } else if (st == 1u) {
                if (dig) { nd++; val = val * 10ull + d; on = nd <= 10u; }
                else { on = b == ',' && nd >= 1u && val >= 1ull && val <= 0x7FFFFFFFull; e->pos = (int64_t)val; st = 2u; }
            } else if (st == 2u) {
                on = b == '+' || b == '-'; e->minus = b == '-'; st = 3u;
            } else if (st == 3u) {
                on = b == ','; st = 4u; nd = 0u; val = 0ull;
            } else if (st == 4u) {
                if (dig) { nd++; val = val * 10ull + d; on = nd <= 9u; }
                else if (nd >= 1u) {
                    // MIDNSHP=X
                    const bool refc = b == 'M' || b == 'D' || b == 'N' || b == '=' || b == 'X', clip = b == 'S' || b == 'H';
                    on = refc || clip || b == 'I' || b == 'P';
                    if (refc) e->span += (int64_t)val;
                    if (b == 'M' || b == 'I' || b == '=' || b == 'X' || clip) e->qlen += (int64_t)val;
                    e->trail = clip ? (uint32_t)val : 0u;
                    if (nops == 0u) e->lead = e->trail;
                    nops++; nd = 0u; val = 0ull;
                } else { on = b == ',' && nops >= 1u; st = 5u; }
            } else if (st == 5u) {
                if (dig) { nd++; val = val * 10ull + d; on = nd <= 3u; }
                else { on = b == ',' && nd >= 1u; e->mapq = (uint32_t)val; st = 6u; nd = 0u; }
            } else if (st == 6u) {
                if (dig) nd = 1u;
                else if (nd >= 1u && b == ';') st = 7u;
                else { ok = nd >= 1u && b == 0u; on = false; }
            } else {
                ok = b == 0u; on = false;
            }
        }
    }
    return ok;
}

struct SplitScatterArgs {
    im_dev_records recs;
    const int32_t* len;
    int32_t n_contigs, min_clip, min_mapq;
    const uint8_t* names;       // the contig-name blob
    KeyedTable tab;
};

// One lane per record.  The front and the CIGAR ends first; a lane whose record has a qualifying clip (almost none of a usual chunk)
// walks its CIGAR, and only such lanes send their wave into the tag walk and the parse.  One ticket draw per workgroup; a workgroup
// without a link ends in front of it.
//
// kOverlap (-H; include/indelminer_amd.h, "Junction overlap"): the lane also sums Q1 on its CIGAR walk, makes d from Q1, the entry's Q2
// and the clips it holds already, and leaves d's code in ovl[] at the slot its link claimed.  Which links are stored, and the tickets,
// are the same in either form; the form without is the kernel as it was.
constexpr int64_t kOverlapMax = 32767;          // |d| beyond it is unknown; the code is d + 32768, 0 = unknown

template <bool kOverlap>
__device__ __forceinline__ void splitlink_scatter(const SplitScatterArgs& A, uint16_t* ovl)
{
    __shared__ uint32_t s_aux[kLinkBlock][kAuxWin / 4];
    const int64_t i = (int64_t)blockIdx.x * kLinkBlock + threadIdx.x;
    RecView r = view_record(A.recs.raw, 0u, 0u);
    if (i < A.recs.n) r = view_record(A.recs.raw, A.recs.rec_off[i], A.recs.rec_off[i + 1]);
    // the front (r.ok: a whole core, and the CIGAR and the start of the aux area inside the record)
    const bool front = r.ok && !(r.flag & (0x4u | 0x100u | 0x200u | 0x400u | 0x800u)) && r.tid >= 0 && r.tid < A.n_contigs && (int32_t)r.mapq >= A.min_mapq;
    const uint32_t n = front ? r.n_cigar : 0u;
    const uint8_t* cig = r.p + r.o_cigar;
    // `first` and `last`, the operations that are not H: which ends are soft clips of min_clip bases
    bool left = false, right = false;
    if (n >= 2u) {
        uint32_t kf = 0, kl = n - 1u;
        while (kf < n && (ld_u32(cig + 4u * kf) & 15u) == 5u) kf++;
        while (kl > kf && (ld_u32(cig + 4u * kl) & 15u) == 5u) kl--;
        if (kf < kl) {
            const uint32_t wf = ld_u32(cig + 4u * kf), wl = ld_u32(cig + 4u * kl);
            left = (wf & 15u) == 4u && (int64_t)(wf >> 4) >= A.min_clip;
            right = (wl & 15u) == 4u && (int64_t)(wl >> 4) >= A.min_clip;
        }
    }
    // refend, and L1 / T1: the leading and the trailing run of S and H
    bool cand = left || right;
    int64_t refend = r.pos, l1 = 0, t1 = 0, q1 = 0;
    if (cand) {
        bool consumes = false, lead = true;
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t cw = ld_u32(cig + 4u * k), op = cw & 15u;
            const int64_t ln = (int64_t)(cw >> 4);
            if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) { consumes = true; refend += ln; }
            if constexpr (kOverlap) q1 += (op == 0u || op == 1u || op == 7u || op == 8u) ? ln : 0;
            if (op == 4u || op == 5u) { t1 += ln; l1 += lead ? ln : 0; }
            else { lead = false; t1 = 0; }
        }
        cand = consumes;
    }
    // the tag and its one entry
    AuxWin w; w.lds = s_aux[threadIdx.x]; w.o0 = 0u;
    uint32_t type = 0;
    const uint32_t o_sa = find_tag(r, w, 'S', 'A', cand, &type);
    SaEntry e;
    bool has = parse_sa(r, w, o_sa + 1u, cand && o_sa != 0u && type == 'Z', &e);
    uint64_t key = 0, payload = 0;
    uint32_t code = 0;
    if (has) {
        has = false;
        const int32_t tid2 = contig_of_name(A.names, r.p + e.o_name, e.name_len, e.name_hash);
        if (tid2 >= 0 && (int32_t)e.mapq >= A.min_mapq && e.span >= 1) {
            const int64_t p2 = e.pos - 1, e2 = p2 + e.span;
            const bool same = e.minus == (((r.flag >> 4) & 1u) != 0u);
            const int64_t l2 = same ? e.lead : e.trail, t2 = same ? e.trail : e.lead;
            const bool behind = l2 > l1 && t2 < t1, infront = l2 < l1 && t2 > t1;
            const int64_t clen = A.len[r.tid];
            int64_t pa = 0;
            uint32_t side_a = 0;
            bool end_a = false;
            if (behind) { end_a = right && refend >= 0 && refend <= clen; pa = refend; side_a = 0u; }
            if (infront) { end_a = left && r.pos >= 0 && r.pos <= clen; pa = r.pos; side_a = 1u; }
            if (end_a && e2 <= (int64_t)A.len[tid2]) {
                // behind on the same strand and in front on the other one continue at the part's start; the other two at its end
                const bool at_start = behind == same;
                const int64_t pb = at_start ? p2 : e2;
                const uint32_t kind = side_a | ((at_start ? 1u : 0u) << 1);
                key = link_key(r.tid, pa >> kLinkBucketShift, kind);
                payload = split_payload(pa, tid2, pb);
                has = true;
                if constexpr (kOverlap) {
                    // Q1 == Q2: both records describe one read.  BEHIND: the primary's part ends at read base Q1 - T1, the other
                    // starts at L2; FRONT: the other ends at Q1 - T2, the primary starts at L1
                    const int64_t d = behind ? (q1 + l1) - l2 : (q1 + l1 + t1 - t2) - l1;
                    if (q1 + l1 + t1 == e.qlen && d >= -kOverlapMax && d <= kOverlapMax) code = (uint32_t)(d + kOverlapMax + 1);
                }
            }
        }
    }
    unsigned long long ticket;
    if (!keyed_block_tickets<kLinkBlock, 1>(A.tab, has ? 1u : 0u, &ticket)) return;
    if (has && keyed_admit(A.tab, ticket)) {
        if constexpr (kOverlap) {
            const uint64_t s = keyed_place_at(A.tab, keyed_home(key, A.tab.log2_slots), key, payload);
            if (s < (1ull << A.tab.log2_slots)) ovl[s] = (uint16_t)code;
        } else {
            keyed_place(A.tab, keyed_home(key, A.tab.log2_slots), key, payload);
        }
    }
}

__global__ __launch_bounds__(kLinkBlock) void splitlink_scatter_kernel(SplitScatterArgs A) { splitlink_scatter<false>(A, nullptr); }
__global__ __launch_bounds__(kLinkBlock) void splitlink_scatter_overlap_kernel(SplitScatterArgs A, uint16_t* ovl) { splitlink_scatter<true>(A, ovl); }

// for callers that name the links themselves, as six columns; a link that fails the rule's range checks is dropped (no ticket)
__global__ __launch_bounds__(kLinkWaveBlock) void splitlink_add_kernel(int32_t n, const int32_t* __restrict__ len, int32_t n_contigs,
                                                                       const int32_t* __restrict__ tid, const int32_t* __restrict__ pos,
                                                                       const uint8_t* __restrict__ side, const int32_t* __restrict__ tid2,
                                                                       const int32_t* __restrict__ pos2, const uint8_t* __restrict__ side2, KeyedTable tab)
{
    const int64_t i = (int64_t)blockIdx.x * kLinkWaveBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t ta = tid[i], tb = tid2[i];
    const int64_t pa = pos[i], pb = pos2[i];
    const uint32_t sa = side[i], sb = side2[i];
    if (ta < 0 || ta >= n_contigs || tb < 0 || tb >= n_contigs || sa > 1u || sb > 1u) return;
    if (pa < 0 || pa > len[ta] || pb < 0 || pb > len[tb]) return;
    const uint64_t key = link_key(ta, pa >> kLinkBucketShift, sa | (sb << 1));
    keyed_insert(tab, keyed_home(key, tab.log2_slots), key, split_payload(pa, tb, pb));
}

// the same with a seventh column, d (-32768: unknown, which is code 0 as it stands), into ovl[] at the slot the link claimed
__global__ __launch_bounds__(kLinkWaveBlock) void splitlink_add_overlap_kernel(int32_t n, const int32_t* __restrict__ len, int32_t n_contigs,
                                                                               const int32_t* __restrict__ tid, const int32_t* __restrict__ pos,
                                                                               const uint8_t* __restrict__ side, const int32_t* __restrict__ tid2,
                                                                               const int32_t* __restrict__ pos2, const uint8_t* __restrict__ side2,
                                                                               const int16_t* __restrict__ d, KeyedTable tab, uint16_t* __restrict__ ovl)
{
    const int64_t i = (int64_t)blockIdx.x * kLinkWaveBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t ta = tid[i], tb = tid2[i];
    const int64_t pa = pos[i], pb = pos2[i];
    const uint32_t sa = side[i], sb = side2[i];
    if (ta < 0 || ta >= n_contigs || tb < 0 || tb >= n_contigs || sa > 1u || sb > 1u) return;
    if (pa < 0 || pa > len[ta] || pb < 0 || pb > len[tb]) return;
    const uint64_t key = link_key(ta, pa >> kLinkBucketShift, sa | (sb << 1));
    if (!keyed_admit(tab, atomicAdd(&tab.counters[0], 1ull))) return;
    const uint64_t s = keyed_place_at(tab, keyed_home(key, tab.log2_slots), key, split_payload(pa, tb, pb));
    if (s < (1ull << tab.log2_slots)) ovl[s] = (uint16_t)((int32_t)d[i] + (int32_t)kOverlapMax + 1);
}

struct SplitCountArgs {
    int32_t nq;
    const int32_t* tid1; const uint8_t* side1; const int32_t* a0; const int32_t* a1;
    const int32_t* tid2; const uint8_t* side2; const int32_t* b0; const int32_t* b1;
    const int32_t* len;
    KeyedTable tab;
    uint32_t* count;
};

// One wave per query (the entry point has held its contigs to the reference and its sides to 0 and 1).  Both intervals are clipped to
// [0, length] of their contig.  A lane's link counts when its payload passes the tidB and the two position tests; the wave sums by
// ballot and popcount.
__global__ __launch_bounds__(kLinkWaveBlock) void splitlink_count_kernel(SplitCountArgs A)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < A.nq; q += nwaves) {
        const int32_t tid1 = A.tid1[q], tid2 = A.tid2[q];
        int64_t a0 = A.a0[q], a1 = A.a1[q], b0 = A.b0[q], b1 = A.b1[q];
        const uint32_t kind = (uint32_t)A.side1[q] | ((uint32_t)A.side2[q] << 1);
        const bool in_a = link_clip(&a0, &a1, A.len[tid1]), in_b = link_clip(&b0, &b1, A.len[tid2]);
        uint32_t n = 0;
        if (in_a && in_b) {
            link_walk(A.tab, tid1, kind, a0, a1, lane, [&](bool has, int64_t bucket, uint64_t payload) {
                const int64_t pa = (bucket << kLinkBucketShift) | (int64_t)(payload & 255ull), pb = (int64_t)(uint32_t)(payload >> 32);
                const int32_t tb = (int32_t)(((uint32_t)payload >> 8) & 0xFFFFFFu);
                const bool counts = has && pa >= a0 && pa <= a1 && tb == tid2 && pb >= b0 && pb <= b1;
                n += (uint32_t)__builtin_popcountll(__ballot(counts));
            });
        }
        if (lane == 0) A.count[q] = n;
    }
}

// ---- the junctions of the split links alone (-J): include/indelminer_amd.h, "Split junctions", has the rule ----------

// A stored link, out of its slot's two words
struct SplitLink {
    int32_t ta, tb;
    int64_t pa, pb;
    uint32_t sa, sb;
};

__device__ __forceinline__ SplitLink split_decode(uint64_t key, uint64_t payload)
{
    SplitLink l;
    l.ta = (int32_t)((key >> 26) & 0xFFFFFFull); l.tb = (int32_t)(((uint32_t)payload >> 8) & 0xFFFFFFu);
    l.pa = (int64_t)(((key >> 2) & 0xFFFFFFull) << kLinkBucketShift) | (int64_t)(payload & 255ull); l.pb = (int64_t)(uint32_t)(payload >> 32);
    l.sa = (uint32_t)key & 1u; l.sb = ((uint32_t)key >> 1) & 1u;
    return l;
}

// rev, can and the candidate test of the rule
__device__ __forceinline__ SplitLink split_rev(const SplitLink& l) { return SplitLink{l.tb, l.ta, l.pb, l.pa, l.sb, l.sa}; }

__device__ __forceinline__ bool split_is_can(const SplitLink& l)
{
    if (l.ta != l.tb) return l.ta < l.tb;
    if (l.pa != l.pb) return l.pa < l.pb;
    return l.sa <= l.sb;
}

__device__ __forceinline__ SplitLink split_can(const SplitLink& l) { return split_is_can(l) ? l : split_rev(l); }

__device__ __forceinline__ bool split_candidate(const SplitLink& l, int64_t min_span)
{
    const int64_t d = l.pa > l.pb ? l.pa - l.pb : l.pb - l.pa;
    return l.ta != l.tb || d >= min_span;
}

constexpr uint32_t kJuncEmitter = 1u << 31;     // a slot index is below 2^30

// The links from end A = (ta, sa, pa +- window) to end B = (tb, sb, pb +- window), by the whole wave: the one to three buckets of A's
// window, both windows clipped to their contig (what splitlink_count_kernel does with a query).  each(has, slot, l) is called for
// every batch that holds a link of A's buckets and kind; has says whether this lane's slot does, l is that link (zeros without), and
// the link is INSIDE both windows iff in(l).  Every branch is the wave's; the loops are bounded by the bucket and the slot count.
struct SplitEnds {
    int32_t ta, tb;
    uint32_t kind;
    int64_t a0, a1, b0, b1;
    __device__ __forceinline__ bool in(const SplitLink& l) const { return l.pa >= a0 && l.pa <= a1 && l.tb == tb && l.pb >= b0 && l.pb <= b1; }
};

__device__ __forceinline__ SplitEnds split_ends(const SplitJuncArgs& A, int32_t ta, int64_t pa, uint32_t sa, int32_t tb, int64_t pb, uint32_t sb)
{
    SplitEnds e;
    e.ta = ta; e.tb = tb; e.kind = sa | (sb << 1);
    e.a0 = pa - A.window; e.a1 = pa + A.window; e.b0 = pb - A.window; e.b1 = pb + A.window;
    (void)link_clip(&e.a0, &e.a1, A.len[ta]);       // a stored position lies in [0, length]: something is left of both
    (void)link_clip(&e.b0, &e.b1, A.len[tb]);
    return e;
}

template <class Each>
__device__ __forceinline__ void split_walk(const KeyedTable& T, const SplitEnds& e, int lane, Each each)
{
    for (int64_t bucket = e.a0 >> kLinkBucketShift; bucket <= (e.a1 >> kLinkBucketShift); bucket++) {
        const uint64_t want = link_key(e.ta, bucket, e.kind);
        (void)keyed_walk(T, keyed_home(want, T.log2_slots), [want](uint64_t key) { return key == want; }, lane,
                         [&](bool has, uint64_t key, uint64_t s) { each(has, (uint32_t)s, split_decode(has ? key : 0ull, has ? T.slots[2ull * s + 1ull] : 0ull)); });
    }
}

// 1. The sweep: one lane per slot; the occupied ones take a place in the list, on ranks their workgroup draws with one atomic add.
__global__ __launch_bounds__(kLinkBlock) void splitjunc_sweep_kernel(SplitJuncArgs A)
{
    const uint64_t s = (uint64_t)blockIdx.x * kLinkBlock + threadIdx.x;
    const bool used = s < (1ull << A.tab.log2_slots) && A.tab.slots[2ull * s] != 0ull;
    unsigned long long at;
    if (!block_tickets<kLinkBlock, 1>(&A.counters[0], used ? 1u : 0u, &at)) return;
    if (used && at < (unsigned long long)A.n_list) A.list[at] = (uint32_t)s;
}

// 2. One wave per listed link.  A link that is no candidate is done at once.  The others walk the buckets around their own end and,
// under the swapped kind, around their far end, and leave E at their slot, the two window counts at their place in the list, and --
// one link per distinct junction -- the emitter mark: among the links equal to it, the one in the lowest slot; a link that is not
// canonical only while no link equal to its reverse is stored.
__global__ __launch_bounds__(kLinkWaveBlock) void splitjunc_count_kernel(SplitJuncArgs A)
{
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const unsigned long long listed = A.counters[0];
    const uint32_t n = listed < (unsigned long long)A.n_list ? (uint32_t)listed : A.n_list;
    for (uint32_t i = wave; i < n; i += nwaves) {
        const uint32_t s = A.list[i];
        const SplitLink l = split_decode(A.tab.slots[2ull * s], A.tab.slots[2ull * s + 1ull]);
        if (!split_candidate(l, A.min_span)) continue;                 // the wave's: every lane holds the same link
        uint32_t n_own = 0, n_far = 0, eq_own = 0, eq_far = 0, lower = 0;
        const SplitEnds own = split_ends(A, l.ta, l.pa, l.sa, l.tb, l.pb, l.sb), far = split_ends(A, l.tb, l.pb, l.sb, l.ta, l.pa, l.sa);
        split_walk(A.tab, own, lane, [&](bool has, uint32_t slot, const SplitLink& m) {
            const bool eq = has && m.pa == l.pa && m.tb == l.tb && m.pb == l.pb;
            n_own += (uint32_t)__builtin_popcountll(__ballot(has && own.in(m)));
            eq_own += (uint32_t)__builtin_popcountll(__ballot(eq));
            lower += (uint32_t)__builtin_popcountll(__ballot(eq && slot < s));
        });
        split_walk(A.tab, far, lane, [&](bool has, uint32_t, const SplitLink& m) {
            n_far += (uint32_t)__builtin_popcountll(__ballot(has && far.in(m)));
            eq_far += (uint32_t)__builtin_popcountll(__ballot(has && m.pa == l.pb && m.tb == l.ta && m.pb == l.pa));
        });
        const bool own_rev = l.ta == l.tb && l.pa == l.pb && l.sa == l.sb;      // rev(l) == l: the second walk met the first one's links
        const bool emits = lower == 0u && (split_is_can(l) || eq_far == 0u);
        if (lane == 0) {
            A.exact[s] = own_rev ? eq_own : eq_own + eq_far;
            A.n_own[i] = n_own; A.n_far[i] = n_far;
            if (emits) A.list[i] = s | kJuncEmitter;
        }
    }
}

// 3. One wave per 64 places of the list, a lane each: the emitters whose counts reach min_links are taken one by one.  The wave walks
// the same runs again for the candidates near the emitter's junction, reads their E and decides the peak; the surviving lanes take
// their rows through one ballot and one atomic add.  An emitter below min_links needs no walk: it is dropped whatever the walk says,
// and the others find its E at its slot all the same.
__global__ __launch_bounds__(kLinkWaveBlock) void splitjunc_peak_kernel(SplitJuncArgs A)
{
    const int lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
    const unsigned long long listed = A.counters[0];
    const uint32_t n = listed < (unsigned long long)A.n_list ? (uint32_t)listed : A.n_list;
    const int64_t w = A.window;
    for (uint32_t base = wave * 64u; base < n; base += nwaves * 64u) {
        const uint32_t i = base + (uint32_t)lane;
        const uint32_t mark = i < n ? A.list[i] : 0u, s = mark & ~kJuncEmitter;
        SplitLink c = SplitLink{0, 0, 0, 0, 0u, 0u};
        uint32_t e = 0, n1 = 0, n2 = 0;
        if (mark & kJuncEmitter) {
            const SplitLink l = split_decode(A.tab.slots[2ull * s], A.tab.slots[2ull * s + 1ull]);
            const bool is_can = split_is_can(l);
            c = split_can(l); e = A.exact[s];
            n1 = is_can ? A.n_own[i] : A.n_far[i]; n2 = is_can ? A.n_far[i] : A.n_own[i];
        }
        uint64_t todo = __ballot((mark & kJuncEmitter) != 0u && (uint64_t)n1 + (uint64_t)n2 >= (uint64_t)A.min_links), peaks = 0ull;
        for (int turn = 0; turn < 64 && todo; turn++) {                 // the wave's: todo is a ballot
            const int j = (int)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            SplitLink x;
            x.ta = __shfl(c.ta, j); x.tb = __shfl(c.tb, j); x.sa = (uint32_t)__shfl((int)c.sa, j); x.sb = (uint32_t)__shfl((int)c.sb, j);
            x.pa = (int64_t)(uint32_t)__shfl((int)(uint32_t)c.pa, j); x.pb = (int64_t)(uint32_t)__shfl((int)(uint32_t)c.pb, j);
            const uint32_t xe = (uint32_t)__shfl((int)e, j);
            bool beaten = false;
            const auto meet = [&](bool has, uint32_t slot, const SplitLink& m) {
                const SplitLink y = split_can(m);
                const bool near_x = has && split_candidate(m, A.min_span) && y.ta == x.ta && y.sa == x.sa && y.tb == x.tb && y.sb == x.sb &&
                                    y.pa >= x.pa - w && y.pa <= x.pa + w && y.pb >= x.pb - w && y.pb <= x.pb + w;
                const uint32_t ye = near_x ? A.exact[slot] : 0u;
                const bool beats = near_x && (ye > xe || (ye == xe && (y.pa < x.pa || (y.pa == x.pa && y.pb < x.pb))));
                beaten = beaten || __ballot(beats) != 0ull;
            };
            split_walk(A.tab, split_ends(A, x.ta, x.pa, x.sa, x.tb, x.pb, x.sb), lane, meet);
            split_walk(A.tab, split_ends(A, x.tb, x.pb, x.sb, x.ta, x.pa, x.sa), lane, meet);
            if (!beaten) peaks |= 1ull << j;
        }
        if (!peaks) continue;                                           // the wave's
        unsigned long long first = 0ull;
        if (lane == 0) first = atomicAdd(&A.counters[1], (unsigned long long)__builtin_popcountll(peaks));
        first = (unsigned long long)(uint64_t)uni64((int64_t)first);
        const unsigned long long row = first + (unsigned long long)__builtin_popcountll(peaks & ((1ull << lane) - 1ull));
        if (((peaks >> lane) & 1ull) && row < (unsigned long long)A.cap) {
            A.col[0][row] = (uint32_t)c.ta; A.col[1][row] = (uint32_t)c.pa; A.col[2][row] = c.sa;
            A.col[3][row] = (uint32_t)c.tb; A.col[4][row] = (uint32_t)c.pb; A.col[5][row] = c.sb;
            A.col[6][row] = e; A.col[7][row] = n1; A.col[8][row] = n2;
        }
    }
}

// ---- the overlap of a junction's links (-H): include/indelminer_amd.h, "Junction overlap", has the rule ----------

// One wave per junction.  D is the codes (ovl[]: d + 32768, 0 = unknown) of the links that the two window counts of rule 5 count: those
// from the window around end 1 to the one around end 2 and those the other way round, a link that both count taken once.  The lower
// median is found by bisection over the 16-bit code, not by sorting: a pass walks the same probe runs again and counts the codes in
// [from, to] by ballot and popcount, so a site of thousands of links needs no memory at all.  Pass 0 counts D; passes 1 .. 16 halve
// [lo, hi] around the smallest code c with #(codes <= c) >= (|D| - 1) / 2 + 1; pass 17 counts the codes equal to it.  Every branch is
// on values the whole wave shares; the loops are bounded by the pass, the bucket and the slot count.
__global__ __launch_bounds__(kLinkWaveBlock) void splitlink_overlap_kernel(SplitOverlapArgs A)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < A.nq; q += nwaves) {
        const int32_t t1 = A.tid1[q], t2 = A.tid2[q];
        const int64_t p1 = A.pos1[q], p2 = A.pos2[q];
        const uint32_t s1 = A.side1[q], s2 = A.side2[q];
        SplitEnds fwd, bwd;
        fwd.ta = t1; fwd.tb = t2; fwd.kind = s1 | (s2 << 1);
        fwd.a0 = p1 - A.window; fwd.a1 = p1 + A.window; fwd.b0 = p2 - A.window; fwd.b1 = p2 + A.window;
        // both are one test: the second query's intervals are the first one's, exchanged
        const bool any = link_clip(&fwd.a0, &fwd.a1, A.len[t1]) && link_clip(&fwd.b0, &fwd.b1, A.len[t2]);
        bwd.ta = t2; bwd.tb = t1; bwd.kind = s2 | (s1 << 1);
        bwd.a0 = fwd.b0; bwd.a1 = fwd.b1; bwd.b0 = fwd.a0; bwd.b1 = fwd.a1;
        const bool twice = bwd.ta == fwd.ta && bwd.kind == fwd.kind;       // only then can a link be one of both queries
        uint32_t known = 0, need = 0, agree = 0, lo = 1u, hi = 65535u;
        for (int pass = 0; any && pass < 18; pass++) {
            if (pass >= 1 && pass <= 16 && lo == hi) continue;
            const uint32_t from = pass == 17 ? lo : 1u, to = pass == 0 ? 65535u : pass == 17 ? lo : (lo + hi) >> 1;
            uint32_t n = 0;
            split_walk(A.tab, fwd, lane, [&](bool has, uint32_t slot, const SplitLink& m) {
                const uint32_t code = has && fwd.in(m) ? (uint32_t)A.ovl[slot] : 0u;
                n += (uint32_t)__builtin_popcountll(__ballot(code >= from && code <= to));
            });
            split_walk(A.tab, bwd, lane, [&](bool has, uint32_t slot, const SplitLink& m) {
                const uint32_t code = has && bwd.in(m) && !(twice && fwd.in(m)) ? (uint32_t)A.ovl[slot] : 0u;
                n += (uint32_t)__builtin_popcountll(__ballot(code >= from && code <= to));
            });
            if (pass == 0) {
                known = n; need = (n - 1u) / 2u + 1u;
                if (n == 0u) break;
            } else if (pass <= 16) {
                if (n >= need) hi = to; else lo = to + 1u;
            } else {
                agree = n;
            }
        }
        if (lane == 0) { A.known[q] = known; A.median[q] = known ? (int32_t)lo - 32768 : 0; A.agree[q] = agree; }
    }
}

// ---- the read pairs on either side of a junction (-E): include/indelminer_amd.h, "Junction pairs", has the rule ----------

// The window of an end (p, side) on a contig of clen bases: the reads that support it start inside, in front of p for right clips
// (side 0) and behind it for left clips (side 1); whether anything is left of it behind the clip
__device__ __forceinline__ bool junc_window(int64_t p, uint32_t side, int64_t reach, int64_t back, int64_t clen, int64_t* w0, int64_t* w1)
{
    *w0 = side ? p - back : p - reach;
    *w1 = side ? p + reach : p + back;
    return link_clip(w0, w1, clen);
}

// One wave per junction.  Both ends on one contig: the pair links (payload pos | mpos << 32) of the kind that the sides of the lower
// and the upper end name, pos in the lower end's window, mpos in the upper end's, min_sep apart; pe2 = 0.  Ends on two contigs: the
// mate links (pos = bucket << 8 | payload & 255; mtid, mpos in the payload) stored at end 1's contig that lie in end 1's window and
// point into end 2's, and the same from end 2.  Which table a junction reads is the wave's (every lane holds the same junction), and so
// is every branch around a ballot; the loops are bounded by the bucket count (reach + back <= 65 535: 257 at the most) and the slot
// count.  The sums are by ballot and popcount; lane 0 stores.
__global__ __launch_bounds__(kLinkWaveBlock) void junction_pairs_kernel(JuncPairArgs A)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < A.nq; q += nwaves) {
        const int32_t t1 = A.tid1[q], t2 = A.tid2[q];
        const int64_t p1 = A.pos1[q], p2 = A.pos2[q];
        const uint32_t s1 = A.side1[q], s2 = A.side2[q];
        uint32_t n1 = 0, n2 = 0;
        if (t1 == t2) {
            // lo: the end with the smaller position, end 1 on a tie
            const bool first = p1 <= p2;
            const int64_t plo = first ? p1 : p2, phi = first ? p2 : p1;
            const uint32_t slo = first ? s1 : s2, shi = first ? s2 : s1;
            const uint32_t kind = slo ? (shi ? 2u : 0u) : (shi ? 3u : 1u);
            int64_t a0, a1, b0, b1;
            const bool in_a = junc_window(plo, slo, A.reach, A.back, A.len[t1], &a0, &a1);
            const bool in_b = junc_window(phi, shi, A.reach, A.back, A.len[t1], &b0, &b1);
            if (in_a && in_b) {
                link_walk(A.pair, t1, kind, a0, a1, lane, [&](bool has, int64_t, uint64_t payload) {
                    const int64_t pos = (int64_t)(uint32_t)payload, mpos = (int64_t)(uint32_t)(payload >> 32);
                    const bool counts = has && pos >= a0 && pos <= a1 && mpos >= b0 && mpos <= b1 && mpos - pos >= (int64_t)A.min_sep;
                    n1 += (uint32_t)__builtin_popcountll(__ballot(counts));
                });
            }
        } else {
            int64_t a0, a1, b0, b1;
            const bool in_a = junc_window(p1, s1, A.reach, A.back, A.len[t1], &a0, &a1);
            const bool in_b = junc_window(p2, s2, A.reach, A.back, A.len[t2], &b0, &b1);
            if (in_a && in_b) {
                link_walk(A.mate, t1, s1 | (s2 << 1), a0, a1, lane, [&](bool has, int64_t bucket, uint64_t payload) {
                    const int64_t pos = (bucket << kLinkBucketShift) | (int64_t)(payload & 255ull), mpos = (int64_t)(uint32_t)(payload >> 32);
                    const int32_t mt = (int32_t)(((uint32_t)payload >> 8) & 0xFFFFFFu);
                    const bool counts = has && pos >= a0 && pos <= a1 && mt == t2 && mpos >= b0 && mpos <= b1;
                    n1 += (uint32_t)__builtin_popcountll(__ballot(counts));
                });
                link_walk(A.mate, t2, s2 | (s1 << 1), b0, b1, lane, [&](bool has, int64_t bucket, uint64_t payload) {
                    const int64_t pos = (bucket << kLinkBucketShift) | (int64_t)(payload & 255ull), mpos = (int64_t)(uint32_t)(payload >> 32);
                    const int32_t mt = (int32_t)(((uint32_t)payload >> 8) & 0xFFFFFFu);
                    const bool counts = has && pos >= b0 && pos <= b1 && mt == t1 && mpos >= a0 && mpos <= a1;
                    n2 += (uint32_t)__builtin_popcountll(__ballot(counts));
                });
            }
        }
        if (lane == 0) { A.pe1[q] = n1; A.pe2[q] = n2; }
    }
}

template <class Kernel>
hipError_t launch_link_scatter(Kernel kernel, const RefDev& ref, int32_t min_mapq, const im_dev_records& recs, const KeyedTable& tab, hipStream_t stream)
{
    if (recs.n <= 0) return hipSuccess;
    LinkScatterArgs A;
    A.recs = recs; A.len = ref.len; A.n_contigs = ref.n_contigs; A.min_mapq = min_mapq; A.tab = tab;
    hipLaunchKernelGGL(kernel, dim3((recs.n + kLinkBlock - 1) / kLinkBlock), dim3(kLinkBlock), 0, stream, A);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pairlink_scatter(const RefDev& ref, int32_t min_mapq, const im_dev_records& recs, const KeyedTable& tab, hipStream_t stream)
{
    return launch_link_scatter(pairlink_scatter_kernel, ref, min_mapq, recs, tab, stream);
}

hipError_t launch_pairlink_scatter_stretched(const RefDev& ref, int32_t min_mapq, const im_dev_records& recs, const KeyedTable& tab, hipStream_t stream)
{
    return launch_link_scatter(pairlink_scatter_stretched_kernel, ref, min_mapq, recs, tab, stream);
}

hipError_t launch_junction_pairs(const JuncPairArgs& A, hipStream_t stream)
{
    if (A.nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(junction_pairs_kernel, dim3(wave_grid(A.nq)), dim3(kLinkWaveBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_matelink_scatter(const RefDev& ref, int32_t min_mapq, const im_dev_records& recs, const KeyedTable& tab, hipStream_t stream)
{
    return launch_link_scatter(matelink_scatter_kernel, ref, min_mapq, recs, tab, stream);
}

hipError_t launch_pairlink_add(int32_t n, int32_t tid, int64_t clen, const int32_t* pos, const int32_t* mpos, const uint8_t* kind,
                               const KeyedTable& tab, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pairlink_add_kernel, dim3((n + kLinkWaveBlock - 1) / kLinkWaveBlock), dim3(kLinkWaveBlock), 0, stream, n, tid, clen, pos, mpos, kind, tab);
    return hipGetLastError();
}

hipError_t launch_matelink_add(const RefDev& ref, int32_t n, int32_t tid, const int32_t* pos, const int32_t* mtid, const int32_t* mpos,
                               const uint8_t* kind, const KeyedTable& tab, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(matelink_add_kernel, dim3((n + kLinkWaveBlock - 1) / kLinkWaveBlock), dim3(kLinkWaveBlock), 0, stream, n, tid, ref.len, ref.n_contigs,
                       pos, mtid, mpos, kind, tab);
    return hipGetLastError();
}

hipError_t launch_pairlink_count(int32_t nq, int32_t tid, const uint8_t* kind, const int32_t* a0, const int32_t* a1, const int32_t* b0,
                                 const int32_t* b1, int32_t min_sep, int64_t clen, const KeyedTable& tab, uint32_t* count, hipStream_t stream)
{
    if (nq <= 0) return hipSuccess;
    LinkCountArgs A;
    A.nq = nq; A.tid = tid; A.min_sep = min_sep; A.kind = kind; A.a0 = a0; A.a1 = a1; A.b0 = b0; A.b1 = b1; A.clen = clen; A.tab = tab; A.count = count;
    hipLaunchKernelGGL(pairlink_count_kernel, dim3(wave_grid(nq)), dim3(kLinkWaveBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_matelink_partner(int32_t nq, int32_t tid, const uint8_t* kind, const int32_t* a0, const int32_t* a1, int64_t clen,
                                   const KeyedTable& tab, uint32_t* n_links, int32_t* mtid, uint32_t* n_partner, int32_t* lo, int32_t* hi,
                                   hipStream_t stream)
{
    if (nq <= 0) return hipSuccess;
    MatePartnerArgs A;
    A.nq = nq; A.tid = tid; A.kind = kind; A.a0 = a0; A.a1 = a1; A.clen = clen; A.tab = tab;
    A.n_links = n_links; A.mtid = mtid; A.n_partner = n_partner; A.lo = lo; A.hi = hi;
    hipLaunchKernelGGL(matelink_partner_kernel, dim3(wave_grid(nq)), dim3(kLinkWaveBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_splitlink_scatter(const RefDev& ref, int32_t min_clip, int32_t min_mapq, const uint8_t* names, const im_dev_records& recs,
                                    const KeyedTable& tab, hipStream_t stream)
{
    if (recs.n <= 0) return hipSuccess;
    SplitScatterArgs A;
    A.recs = recs; A.len = ref.len; A.n_contigs = ref.n_contigs; A.min_clip = min_clip; A.min_mapq = min_mapq; A.names = names; A.tab = tab;
    hipLaunchKernelGGL(splitlink_scatter_kernel, dim3((recs.n + kLinkBlock - 1) / kLinkBlock), dim3(kLinkBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_splitlink_add(const RefDev& ref, int32_t n, const int32_t* tid, const int32_t* pos, const uint8_t* side, const int32_t* tid2,
                                const int32_t* pos2, const uint8_t* side2, const KeyedTable& tab, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(splitlink_add_kernel, dim3((n + kLinkWaveBlock - 1) / kLinkWaveBlock), dim3(kLinkWaveBlock), 0, stream, n, ref.len, ref.n_contigs,
                       tid, pos, side, tid2, pos2, side2, tab);
    return hipGetLastError();
}

hipError_t launch_splitlink_scatter_overlap(const RefDev& ref, int32_t min_clip, int32_t min_mapq, const uint8_t* names, const im_dev_records& recs,
                                            const KeyedTable& tab, uint16_t* ovl, hipStream_t stream)
{
    if (recs.n <= 0) return hipSuccess;
    SplitScatterArgs A;
    A.recs = recs; A.len = ref.len; A.n_contigs = ref.n_contigs; A.min_clip = min_clip; A.min_mapq = min_mapq; A.names = names; A.tab = tab;
    hipLaunchKernelGGL(splitlink_scatter_overlap_kernel, dim3((recs.n + kLinkBlock - 1) / kLinkBlock), dim3(kLinkBlock), 0, stream, A, ovl);
    return hipGetLastError();
}

hipError_t launch_splitlink_add_overlap(const RefDev& ref, int32_t n, const int32_t* tid, const int32_t* pos, const uint8_t* side, const int32_t* tid2,
                                        const int32_t* pos2, const uint8_t* side2, const int16_t* d, const KeyedTable& tab, uint16_t* ovl,
                                        hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(splitlink_add_overlap_kernel, dim3((n + kLinkWaveBlock - 1) / kLinkWaveBlock), dim3(kLinkWaveBlock), 0, stream, n, ref.len,
                       ref.n_contigs, tid, pos, side, tid2, pos2, side2, d, tab, ovl);
    return hipGetLastError();
}

hipError_t launch_splitlink_overlap(const SplitOverlapArgs& A, hipStream_t stream)
{
    if (A.nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(splitlink_overlap_kernel, dim3(wave_grid(A.nq)), dim3(kLinkWaveBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_splitlink_count(const RefDev& ref, int32_t nq, const int32_t* tid1, const uint8_t* side1, const int32_t* a0, const int32_t* a1,
                                  const int32_t* tid2, const uint8_t* side2, const int32_t* b0, const int32_t* b1, const KeyedTable& tab,
                                  uint32_t* count, hipStream_t stream)
{
    if (nq <= 0) return hipSuccess;
    SplitCountArgs A;
    A.nq = nq; A.tid1 = tid1; A.side1 = side1; A.a0 = a0; A.a1 = a1; A.tid2 = tid2; A.side2 = side2; A.b0 = b0; A.b1 = b1; A.len = ref.len;
    A.tab = tab; A.count = count;
    hipLaunchKernelGGL(splitlink_count_kernel, dim3(wave_grid(nq)), dim3(kLinkWaveBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_splitlink_junctions(const SplitJuncArgs& A, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(A.counters, 0, 2 * sizeof(unsigned long long), stream);
    if (e != hipSuccess || A.n_list == 0u) return e;
    const uint64_t slots = 1ull << A.tab.log2_slots;
    hipLaunchKernelGGL(splitjunc_sweep_kernel, dim3((unsigned)((slots + kLinkBlock - 1) / kLinkBlock)), dim3(kLinkBlock), 0, stream, A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(splitjunc_count_kernel, dim3(wave_grid(A.n_list)), dim3(kLinkWaveBlock), 0, stream, A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(splitjunc_peak_kernel, dim3(wave_grid(((int64_t)A.n_list + 63) / 64)), dim3(kLinkWaveBlock), 0, stream, A);
    return hipGetLastError();
}

}  // namespace im
