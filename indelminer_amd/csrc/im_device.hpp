// im_device.hpp -- shared declarations of the HIP side (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "indelminer_amd.h"

namespace im {

// Reference contigs resident in HBM, two forms:
//   ascii : the bytes as the reference keeps them (src/shared.c:46-82); each
//           contig starts 256-byte aligned with >= 64 zero bytes before and
//           after, so unaligned 4/16-byte reads at a window edge stay in bounds.
//           Needed by the diagonal scan, which compares raw bytes
//           (W[i][j] = MATCH iff i == j, src/localalign.c:61-67).
//   pk    : 2-bit codes (base2bits, src/alignment.c:11-24: A,a=0 C,c=1 G,g=2
//           T,t=3, anything else 0), 4 bases per byte, first base in the least
//           significant bits, so an unaligned dword at byte p/4 shifted right by
//           2*(p%4) starts with the k-mer at p.  >= 1 KiB of zero bytes follow the
//           last contig (the vote reads up to a sweep past a window).  Needed by
//           the k-mer band vote only.
struct RefDev {
    const uint8_t*  ascii;
    const uint8_t*  pk;
    const int64_t*  asc_off;    // [n_contigs] byte offset of contig start in ascii
    const int64_t*  pk_off;     // [n_contigs] byte offset of contig start in pk
    const int32_t*  len;        // [n_contigs]
    int32_t         n_contigs;
};

constexpr int kShortRead = 255;      // longest read of the four-positions-per-lane kernels (im_realign.hip)
constexpr int kMaxWaveGaps = 60;     // widest numgaps of the lane-per-diagonal band kernel (a band of 61 diagonals and its two borders in one wave)

struct RealignArgs {
    RefDev      ref;
    im_dev_batch batch;
    im_params   P;
    int32_t     keep_slots;     // 1: evidence slots of reads without realigned evidence are left as they are
    const int32_t* n_dev;       // device-resident batch size (null: batch.n), batch.n is then the upper bound
    int32_t     first;          // realign_kernel: the first read of this launch's slice (launch_realign cuts a batch beyond its largest grid)
};

// The read-group -> range[1] table of the insert-length hashtable, flattened into one blob:
// int32 bin_start[20] (17 used; 16 bins of the qhash of size 2^4, src/indelminer.c:702), name_off[m], name_len[m],
// range_max[m] (m = max(n,1); the entries of a bin in chain order, head first), then the names.
struct RgTable {
    const uint8_t* blob;
    int32_t n;
    int32_t bytes;
    // must_find_hashtable(insertlengths, "generic") (records without an RG tag, src/indelminer.c:370), looked up once on the
    // host when the table is set: the table does not change until the next im_set_insert_ranges
    int32_t generic_ok, generic_range;
};

size_t triage_scratch_bytes(int32_t n_records);
size_t triage_scratch_zero_offset(int32_t n_records, size_t* bytes);
hipError_t launch_triage(const RefDev& ref, const RgTable& rg, int32_t* depth_diff, const im_triage_params& tp,
                         const im_dev_records& recs, const im_dev_cands& out, void* scratch, hipStream_t stream);

hipError_t launch_flush_cut(const int32_t* cls, const int32_t* b1, const int32_t* b2, int32_t* consumed,
                            int32_t a0, int32_t a1, int32_t b0, int32_t b1_end, int32_t marker, int32_t flush_id,
                            uint64_t* cut_word, const int32_t* cand_rec, const int32_t* n_cand_dev, int32_t cand_cap, hipStream_t stream);
hipError_t launch_flush_seq(const im_flush_desc* desc, int32_t n_fl, const int32_t* cls, const int32_t* b1, const int32_t* b2,
                            int32_t* consumed, const int32_t* cand_rec, const int32_t* n_cand_dev, int32_t cand_cap, int32_t pe_base,
                            int32_t pe_count, hipStream_t stream);
size_t groupby_scratch_bytes(int32_t n_slots);
hipError_t launch_groupby_init(int32_t n_slots, void* scratch, hipStream_t stream);
hipError_t launch_groupby(int32_t n_layout, int32_t n_slots, const int32_t* n_cand_dev, const int32_t* cls, const int32_t* b1, const int32_t* b2, const int32_t* consumed,
                          int32_t tie_desc, int32_t* order, int32_t* cl_key, int32_t* cl_first, int32_t* cl_count,
                          int32_t* counts, void* scratch, hipStream_t stream);
// im_flushwide.hip: the flush list and the group-by chip-wide (three launches)
size_t flushgroup_scratch_bytes(int32_t n_slots, int32_t n_fl_cap);
hipError_t launch_flushgroup_init(int32_t n_slots, int32_t n_fl_cap, void* scratch, hipStream_t stream);
hipError_t launch_flush_groupby(int32_t n_slots_layout, int32_t n_fl_layout, const im_flush_desc* desc, int32_t n_fl,
                                const int32_t* cls, const int32_t* b1, const int32_t* b2, int32_t* consumed,
                                const int32_t* cand_rec, const int32_t* n_cand_dev, int32_t cand_cap, int32_t pe_base, int32_t pe_count,
                                int32_t tie_desc, int32_t* order, int32_t* cl_key, int32_t* cl_first, int32_t* cl_count, int32_t* counts,
                                void* scratch, hipStream_t stream);

// im_depth.hip: a contig's difference array (clen + 1 ints: the depth array, the span array) and its tile sums; the file's header
// has the one rule for sums.  After the scan the array is tile-local: the value at p is data[p] + sums[p / kScanTile].
constexpr int kScanTile = 8192;
int64_t depth_sums_ints(int64_t clen);
hipError_t launch_depth_scan_tiled(int32_t* depth, int64_t n, int32_t* sums, hipStream_t stream);
hipError_t launch_fill_zero(int32_t* p, int64_t n, hipStream_t stream);       // n ints from p (16-byte aligned) to zero, one launch
// memset + interval scatter (+1 at a + lo, -1 at b - hi of every clipped [a, b) with a + lo < b - hi) + scan; zeroes sums itself
hipError_t launch_depth_build(int64_t clen, int32_t n_seg, const int32_t* seg_start, const int32_t* seg_len, int32_t lo, int32_t hi,
                              int32_t* data, int32_t* sums, hipStream_t stream);
// sum over [beg, end); out_max (may be null): the deepest position of [beg - 1, end]
hipError_t launch_depth_query_tiled(int32_t nq, const int32_t* beg, const int32_t* end, const int32_t* depth, const int32_t* sums,
                                    int64_t clen, uint32_t* out, uint32_t* out_max, hipStream_t stream);
// lower median over [beg, end) of min(value, 4095), by histogram: one launch; im_depth.hip has the work items, the scratch and the rule
int32_t depth_median_slabs(int32_t beg, int32_t end, int64_t clen);
size_t depth_median_scratch_bytes(int32_t slots);
hipError_t launch_depth_median(int32_t nq, int32_t items, const int32_t* beg, const int32_t* end, const int32_t* first, const int32_t* slot,
                               const int32_t* data, const int32_t* sums, int64_t clen, uint32_t* scratch, int32_t slots, int32_t max_blocks,
                               uint32_t* out, hipStream_t stream);

// im_realign.hip
hipError_t launch_pack_reference(const uint8_t* ascii, uint64_t* pk, int64_t n_bases_padded,
                                 hipStream_t stream);
hipError_t launch_realign(const RealignArgs& a, int n_cu, hipStream_t stream);
// im_realign_long.hip: the reads of kShortRead + 1 .. IM_MAX_READ bases of the same batch (numgaps == 0)
hipError_t launch_realign_long(const RealignArgs& a, int n_cu, hipStream_t stream);

// im_realign_any.hip: the reads the laid-out kernels leave IM_ST_UNSUPPORTED (any length, any band width), one lane per read.
// pick lists them (all != 0: every read of the batch, which no other kernel has seen) into list[] with counters[0] = how many,
// [1] = the longest read, [2] = the widest window among them; the caller sizes the arena from those (n_waves waves of 64 lanes).
hipError_t launch_realign_any_pick(const RealignArgs& a, int all, int32_t* list, int32_t* counters, hipStream_t stream);
// lane_shift: log2 of the reads a wave holds at a time (6 = every lane; fewer reads per wave = more waves for a small batch)
size_t realign_any_arena_bytes(int32_t max_read, int32_t max_window, uint32_t numgaps, int32_t lane_shift, int32_t n_waves);
hipError_t launch_realign_any(const RealignArgs& a, const int32_t* list, int32_t* counters, int32_t* arena,
                              int32_t max_read, int32_t max_window, int32_t lane_shift, int32_t n_waves, hipStream_t stream);

// im_results.hip
hipError_t launch_compact_results(const im_read_result* res, int32_t n_cap, const int32_t* n_dev, int32_t* status, int32_t* slot,
                                  im_read_result* compact, int32_t* count, int n_cu, hipStream_t stream);

// im_span.hip: reference-spanning read counts (the genotype columns); the array has the depth array's layout, build and scan
hipError_t launch_span_scatter(const RefDev& ref, int32_t flank, int32_t min_mapq, const im_dev_records& recs, int32_t* diff, hipStream_t stream);
// concordant left mates -> fragment events in a difference array of the same layout (rg: the table of im_set_insert_ranges)
hipError_t launch_pair_scatter(const RefDev& ref, const RgTable& rg, int32_t flank, int32_t min_mapq, const im_dev_records& recs, int32_t* diff, hipStream_t stream);
// clipped reads -> point counts in two arrays of that layout: right[refend] and left[pos] (see im_span.hip); never scanned
hipError_t launch_clip_scatter(const RefDev& ref, int32_t min_clip, int32_t min_mapq, const im_dev_records& recs, int32_t* right, int32_t* left,
                               hipStream_t stream);
// memset of both arrays' clen + 1 entries + one count per host-named event (side 0: right, 1: left; positions outside [0, clen] dropped)
hipError_t launch_clip_build(int64_t clen, int32_t n, const int32_t* pos, const uint8_t* side, int32_t* right, int32_t* left, hipStream_t stream);
// per query the largest count over [beg, end] inclusive of right (side 0) or left (side 1) and the smallest position holding it; (0, -1) when empty
hipError_t launch_clip_argmax(int32_t nq, const uint8_t* side, const int32_t* beg, const int32_t* end, const int32_t* right, const int32_t* left,
                              int64_t clen, uint32_t* count_out, int32_t* pos_out, hipStream_t stream);
// the facing piles of one contig's two arrays (clen + 1 entries each, 16-byte aligned): positions pr with right[pr] >= min_reads that
// are a peak of right within max_overlap and have left[pl] >= min_reads for some pl in [pr - max_overlap, pr]; *n_found (cleared here)
// counts them all, the first cap that take a slot are written, in no particular order
hipError_t launch_clip_facing(const int32_t* right, const int32_t* left, int64_t clen, int32_t min_reads, int32_t max_overlap, int32_t cap,
                              int32_t* pr, int32_t* pl, uint32_t* cr, uint32_t* cl, uint32_t* n_found, hipStream_t stream);
// the peaks of ONE array (clen + 1 entries, 16-byte aligned): positions p with arr[p] >= min_reads, arr[p] > every count of
// [p - reach, p) and >= every count of (p, p + reach]; *n_found (cleared here) counts them all, the first cap that take a slot are
// written, in no particular order
hipError_t launch_clip_peaks(const int32_t* arr, int64_t clen, int32_t min_reads, int32_t reach, int32_t cap, int32_t* pos, uint32_t* count,
                             uint32_t* n_found, hipStream_t stream);
// The keyed table behind the clip tails (-V), the pair links (-M), the mate links (-T) and the split links (-S), an allocation each; im_keyed.hpp has its definition.  slots:
// 2^log2_slots pairs (key, payload) of 64-bit words, zeros = empty; counters[0]: inserts asked for, counters[1]: those dropped because
// half of the slots were taken
struct KeyedTable {
    unsigned long long* slots;
    unsigned long long* counters;
    int32_t log2_slots;
};
// im_cliptail.hip: the clipped bases of clipped reads in a keyed table (-V)
// the records that clip under the clip scatter's rule -> one entry per clipping end whose nearest min(clip, 32) bases are all A/C/G/T
hipError_t launch_cliptail_scatter(const RefDev& ref, int32_t min_clip, int32_t min_mapq, const im_dev_records& recs, const KeyedTable& tab,
                                   hipStream_t stream);
// one entry per host-named (position, side, bases, planes[2]: low-bit plane, high-bit plane); positions outside [0, clen] dropped
hipError_t launch_cliptail_add(int32_t n, int32_t tid, int64_t clen, const int32_t* pos, const uint8_t* side, const uint8_t* nbases,
                               const uint32_t* planes, const KeyedTable& tab, hipStream_t stream);
// per query (pr, pl) on contig tid (ref: its ASCII bases): the entries at either key that continue behind the other breakpoint at the
// best shift 0 .. max_shift <= 32, that shift (-1: none matched or pl <= pr), and the entries stored at the two keys
hipError_t launch_cliptail_verify(int32_t nq, int32_t tid, const int32_t* pr, const int32_t* pl, int32_t max_shift, const uint8_t* ref,
                                  int64_t clen, const KeyedTable& tab, uint32_t* v_right, uint32_t* v_left, int32_t* shift,
                                  uint32_t* stored_right, uint32_t* stored_left, hipStream_t stream);
// per query (pos, side) on contig tid: the entries stored at the key, the bases covered by at least min_cover of them, their per-base
// consensus as two planes (planes[2 q], planes[2 q + 1]) and the entries that agree with it; a position outside [0, clen] answers zeros
hipError_t launch_cliptail_consensus(int32_t nq, int32_t tid, const int32_t* pos, const uint8_t* side, int32_t min_cover, int64_t clen,
                                     const KeyedTable& tab, uint32_t* entries, uint32_t* len, uint32_t* planes, uint32_t* agree, hipStream_t stream);
// Pairs of piles whose entries verify: at least min_verified at either pile at the chosen shift 0 .. max_shift <= 32.  Both peak lists
// are ascending.  Crossed (-U): p1 of the right peaks, p2 of the left peaks, min_len <= p1 - p2 <= max_len, against the reference
// behind the other pile; nothing is launched while either list is empty.  Inverted (-N): p1 < p2 of ONE list (side 0: the right peaks,
// 1: the left peaks), min_len <= p2 - p1 <= max_len, against the reference's reverse complement; one launch for both lists, none when
// both are empty.  *n_found (cleared by the launch) counts every pair; the first cap that take a slot are written, in no particular
// order, into ten columns: side (0 for crossed), p1, p2, their counts, v1, v2, shift, stored at p1, stored at p2.
struct TailPairsArgs {
    int32_t n_right, n_left, tid;
    const int32_t* rpos;        // the peaks of clipR, ascending, and their counts
    const uint32_t* rcnt;
    const int32_t* lpos;        // the peaks of clipL, ascending, and their counts
    const uint32_t* lcnt;
    int32_t min_len, max_len, max_shift, min_verified, cap;
    const uint8_t* ref;         // the contig's ASCII bases
    int64_t clen;
    KeyedTable tab;
    uint32_t* col[10];
    uint32_t* n_found;
};
hipError_t launch_cliptail_pairs(bool inverted, TailPairsArgs A, hipStream_t stream);
// im_links.hip: the read pairs of an abnormal orientation in a keyed table of its own (-M)
// the records that are a link under the record rule (include/indelminer_amd.h, "Pair links") -> one entry each
hipError_t launch_pairlink_scatter(const RefDev& ref, int32_t min_mapq, const im_dev_records& recs, const KeyedTable& tab, hipStream_t stream);
// one entry per host-named (pos, mpos, kind 0 .. 2) of contig tid; a position outside [0, clen] drops the link
hipError_t launch_pairlink_add(int32_t n, int32_t tid, int64_t clen, const int32_t* pos, const int32_t* mpos, const uint8_t* kind,
                               const KeyedTable& tab, hipStream_t stream);
// per query (kind, [a0, a1], [b0, b1]) on contig tid, both intervals inclusive and clipped to [0, clen]: the links of that kind with pos
// in the first, mpos in the second and mpos - pos >= min_sep; the caller holds a1 - a0 to 65 535
hipError_t launch_pairlink_count(int32_t nq, int32_t tid, const uint8_t* kind, const int32_t* a0, const int32_t* a1, const int32_t* b0,
                                 const int32_t* b1, int32_t min_sep, int64_t clen, const KeyedTable& tab, uint32_t* count, hipStream_t stream);
// the same with the fourth kind of "Junction pairs" (3 STRETCHED: the normal orientation, not flagged a proper pair); the links of
// kinds 0 .. 2 are those of the form above
hipError_t launch_pairlink_scatter_stretched(const RefDev& ref, int32_t min_mapq, const im_dev_records& recs, const KeyedTable& tab, hipStream_t stream);
// per junction (tid1, pos1, side1, tid2, pos2, side2): the read pairs between the windows of its two ends (include/indelminer_amd.h,
// "Junction pairs") -- on one contig pe1 out of the pair-link table and pe2 = 0, on two contigs pe1 and pe2 out of the mate-link table,
// from either end; the caller holds the contigs to the reference, the sides to 0 and 1, reach, back and min_sep to >= 0 and
// reach + back to 65 535
struct JuncPairArgs {
    int32_t nq, reach, back, min_sep;
    const int32_t* tid1; const int32_t* pos1; const uint8_t* side1;
    const int32_t* tid2; const int32_t* pos2; const uint8_t* side2;
    const int32_t* len;
    KeyedTable pair, mate;
    uint32_t* pe1; uint32_t* pe2;
};
hipError_t launch_junction_pairs(const JuncPairArgs& A, hipStream_t stream);
// im_links.hip: the read pairs whose mate lies on another contig in a keyed table of its own (-T)
// the records that are a link under the record rule (include/indelminer_amd.h, "Mate links") -> one entry each
hipError_t launch_matelink_scatter(const RefDev& ref, int32_t min_mapq, const im_dev_records& recs, const KeyedTable& tab, hipStream_t stream);
// one entry per host-named (pos, mtid, mpos, kind 0 .. 3) of contig tid; a link that fails the rule's range checks is dropped
hipError_t launch_matelink_add(const RefDev& ref, int32_t n, int32_t tid, const int32_t* pos, const int32_t* mtid, const int32_t* mpos,
                               const uint8_t* kind, const KeyedTable& tab, hipStream_t stream);
// per query (kind, [a0, a1]) on contig tid, the interval inclusive and clipped to [0, clen]: the links of that kind inside it, the contig
// and the two neighbouring 1 024-base cells most of their mates lie in, their number and their mates' range (mtid -1: no link, -2: more
// than IM_MATELINK_CELLS cells); the caller holds a1 - a0 to 65 535
hipError_t launch_matelink_partner(int32_t nq, int32_t tid, const uint8_t* kind, const int32_t* a0, const int32_t* a1, int64_t clen,
                                   const KeyedTable& tab, uint32_t* n_links, int32_t* mtid, uint32_t* n_partner, int32_t* lo, int32_t* hi,
                                   hipStream_t stream);
// im_links.hip: the split reads (a soft-clipped primary record and its SA:Z tag) in a keyed table of its own (-S)
// the records that are a link under the record rule (include/indelminer_amd.h, "Split links") -> one entry each; names: the contig-name
// blob of im_splitlink_enable
hipError_t launch_splitlink_scatter(const RefDev& ref, int32_t min_clip, int32_t min_mapq, const uint8_t* names, const im_dev_records& recs,
                                    const KeyedTable& tab, hipStream_t stream);
// one entry per host-named (tid, pos, side, tid2, pos2, side2); a link that fails the rule's range checks is dropped
hipError_t launch_splitlink_add(const RefDev& ref, int32_t n, const int32_t* tid, const int32_t* pos, const uint8_t* side, const int32_t* tid2,
                                const int32_t* pos2, const uint8_t* side2, const KeyedTable& tab, hipStream_t stream);
// per query (tid1, side1, [a0, a1], tid2, side2, [b0, b1]), both intervals inclusive and clipped to [0, length] of their contig: the
// links of kind side1 | side2 << 1 from the first to the second; the caller holds the contigs to the reference, the sides to 0 and 1
// and a1 - a0 to 65 535
hipError_t launch_splitlink_count(const RefDev& ref, int32_t nq, const int32_t* tid1, const uint8_t* side1, const int32_t* a0, const int32_t* a1,
                                  const int32_t* tid2, const uint8_t* side2, const int32_t* b0, const int32_t* b1, const KeyedTable& tab,
                                  uint32_t* count, hipStream_t stream);
// The junctions of the split links alone (include/indelminer_amd.h, "Split junctions"): a sweep lists the occupied slots, a wave per
// listed link counts E and the two windows, a wave per 64 of them decides the peaks.  The caller provides the workspace (counters: two
// words; list, n_own, n_far: n_list words each; exact: a word per SLOT) and nine columns of max(cap, 1) words; the launch clears the
// counters.  counters[1] is the number of junctions, of which the first cap that take a row are written, in no particular order.
struct SplitJuncArgs {
    KeyedTable tab;
    const int32_t* len;
    int32_t window, min_links, min_span, cap;
    uint32_t n_list;                    // the list's length: the links stored (the ticket rule makes it exact)
    unsigned long long* counters;       // [0] the slots listed, [1] the junctions found
    uint32_t* list;                     // n_list: a listed link's slot; bit 31: it is the emitter among its equals
    uint32_t* exact;                    // per SLOT: E of the candidate link it holds
    uint32_t* n_own;                    // n_list: the links from the window around its own end to the window around its far end
    uint32_t* n_far;                    // n_list: the same with the ends exchanged
    uint32_t* col[9];                   // tid1, pos1, side1, tid2, pos2, side2, exact, n1, n2
};
hipError_t launch_splitlink_junctions(const SplitJuncArgs& A, hipStream_t stream);
// The overlap of the split links (include/indelminer_amd.h, "Junction overlap"): ovl is one 16-bit code per SLOT of the table, d + 32768
// or 0 for unknown, written behind the claim of the slot.  The scatter and the add with it store the links, and draw the tickets, that
// the forms without it do.
hipError_t launch_splitlink_scatter_overlap(const RefDev& ref, int32_t min_clip, int32_t min_mapq, const uint8_t* names, const im_dev_records& recs,
                                            const KeyedTable& tab, uint16_t* ovl, hipStream_t stream);
hipError_t launch_splitlink_add_overlap(const RefDev& ref, int32_t n, const int32_t* tid, const int32_t* pos, const uint8_t* side, const int32_t* tid2,
                                        const int32_t* pos2, const uint8_t* side2, const int16_t* d, const KeyedTable& tab, uint16_t* ovl,
                                        hipStream_t stream);
// per junction (tid1, pos1, side1, tid2, pos2, side2): the known codes of the links between the windows of `window` bases around its two
// ends, from either -- their number, their lower median as d, and how many equal it; the caller holds the contigs to the reference, the
// sides to 0 and 1 and window to 0 .. 255
struct SplitOverlapArgs {
    int32_t nq, window;
    const int32_t* tid1; const int32_t* pos1; const uint8_t* side1;
    const int32_t* tid2; const int32_t* pos2; const uint8_t* side2;
    const int32_t* len;
    KeyedTable tab;
    const uint16_t* ovl;
    uint32_t* known; int32_t* median; uint32_t* agree;
};
hipError_t launch_splitlink_overlap(const SplitOverlapArgs& A, hipStream_t stream);
// per query (tid1, p1, side1, tid2, p2, side2): the entries at either end that continue in the OTHER end's contig at the best shift
// 0 .. max_shift <= 32 (include/indelminer_amd.h, "Junctions"), that shift (-1: none matched), and the entries stored at the two keys
struct TailJunctionArgs {
    int32_t nq, max_shift;
    const int32_t* tid1; const int32_t* p1; const uint8_t* side1;
    const int32_t* tid2; const int32_t* p2; const uint8_t* side2;
    RefDev ref;
    KeyedTable tab;
    uint32_t* v1; uint32_t* v2; int32_t* shift; uint32_t* stored1; uint32_t* stored2;
};
hipError_t launch_cliptail_junction(const TailJunctionArgs& A, hipStream_t stream);
// minimum over [beg, end] inclusive of a scanned array (0 for an interval that is empty after the clip to [0, clen])
hipError_t launch_span_query(int32_t nq, const int32_t* beg, const int32_t* end, const int32_t* span, const int32_t* sums,
                             int64_t clen, uint32_t* out, hipStream_t stream);
// the same minimum for a list of ENDS, each on its own contig (include/indelminer_amd.h, "Junction genotypes"): per end the interval
// [pos - slack, pos + slack] clipped to its contig, one lane per end, one launch for all n
struct SpanEndsArgs {
    int32_t n, slack;                   // slack 0 .. 255
    const int32_t* tid;                 // [n]
    const int32_t* pos;                 // [n]
    const int64_t* sums_off;            // [n] where the end's contig keeps its run of tile offsets in sums
    const int64_t* asc_off;             // [n_contigs] where a contig's run starts in span (RefDev's)
    const int32_t* len;                 // [n_contigs]
    int32_t n_contigs;
    const int32_t* span;                // the genome-wide array, scanned contig by contig
    const int32_t* sums;                // the tile offsets of those scans
    uint32_t* out;                      // [n]
};
hipError_t launch_span_query_ends(const SpanEndsArgs& A, hipStream_t stream);

// tasks within IM_MAX_SW_TARGET / IM_MAX_READ run in the LDS form; when the batch holds longer ones (big_grid > 0) a second launch
// with its boundary rows in big_scratch (support_big_scratch_bytes) takes those
size_t support_big_scratch_bytes(int64_t max_target, int64_t max_query, int32_t n_tasks, int32_t* grid_out);
hipError_t launch_support(int32_t n_tasks, const uint8_t* targets, const int64_t* t_off,
                          const uint8_t* queries, const int64_t* q_off, int32_t* out, int64_t max_target, int64_t max_query,
                          void* big_scratch, int32_t big_grid, int n_cu, hipStream_t stream);


// the counting form (im_support_count): the windows come through the splice from the resident reference.  The caller lists the
// tasks beyond the LDS form (support_count_is_big) with the offsets of their windows in big_win (support_count_window bytes each);
// attr_set: the context's "function attribute has been set" flag
int64_t support_count_window(const im_known_variant& v, int32_t rstart, int32_t rstop);
bool support_count_is_big(int64_t window, int64_t query);
int64_t support_count_max_query();
hipError_t launch_support_count(int32_t n_tasks, const im_count_task* tasks, const im_known_variant* vars, const uint8_t* alts, const RefDev& ref,
                                const uint8_t* queries, int32_t* counts, int64_t max_short_target,
                                int32_t n_big, const int32_t* big_idx, const int64_t* big_toff, uint8_t* big_win, int64_t max_big_target,
                                void* big_scratch, int32_t big_grid, bool* attr_set, hipStream_t stream);

}  // namespace im
