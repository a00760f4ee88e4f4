// im_cliptail.hip -- the clipped bases of clipped reads (-V): kept in a keyed table, compared against the reference behind the
// partner breakpoint (gfx950).  The definition is in include/indelminer_amd.h (seam 5, "Clip tails"); DESIGN.md 4.5f has the cost.
//
// A record that clips under -C's rule (im_spanrec.hpp: clip_decide, clip_refend -- the very code of clip_scatter_kernel) stores per
// clipping end ONE ENTRY: the n = min(clip length, 32) read bases nearest the junction, base 0 the nearest, at the key
// (tid, position, side), position = refend for a right clip (side 0) and pos for a left clip (side 1).  Nothing is stored when one
// of the n bases is not A / C / G / T or when the packed bases do not lie inside the record.
//
// THE TABLE is the keyed table of im_keyed.hpp (slots, tickets, claim, walk), with
//   word 0   the key: bit 63 set (an empty slot is 0) | tid << 39 | position << 7 | side << 6 | n           (tid < 2^24, n = 1 .. 32)
//   word 1   the payload: the n bases as 2-bit codes (A 0, C 1, G 2, T 3) in two planes, low bits in bits 0 .. 31, high bits in
//            bits 32 .. 63; bit i of a plane belongs to the base at distance i from the junction
// key >> 6 is what enters the hash: n does not, so every entry of one (tid, position, side) lies on one probe run.
//
//   cliptail_scatter   one lane per delivered record; the ~1 % of lanes that clip read their packed bases and insert, on tickets
//                      their workgroup draws with one atomic add
//   cliptail_add       one lane per entry, for callers that name the events themselves
//   cliptail_verify    one wave per query (tid, pr, pl): see the kernel
//   cliptail_consensus one wave per query (tid, position, side): the per-base consensus of a pile's entries (-I), on the same walk
//   cliptail_pairs     one wave per peak: the peaks the right distance away, verified as above.  <false>: a peak of clipR with the
//                      peaks of clipL in front of it (-U); <true>: a peak of either array with the peaks of the SAME array behind it,
//                      against the reference's reverse complement (-N)

#include "im_keyed.hpp"
#include "im_spanrec.hpp"

namespace im {
namespace {

constexpr int kTailBlock = 1024;      // records of a scatter workgroup: one ticket draw each (see cliptail_scatter_kernel)
constexpr int kTailWaveBlock = 256;   // threads of the add and verify kernels
// An entry holds at most kTailBases bases and a query tries the shifts 0 .. S <= kTailMaxShift, so a comparison reaches at most
// kTailMaxShift + kTailBases = 64 bases behind the partner breakpoint: EXACTLY ONE WAVEFRONT of reference bases per side, one base
// per lane, turned into wave-uniform 64-bit planes by three ballots.  Neither constant can grow without a second window.
constexpr int kTailBases = 32;
constexpr int kTailMaxShift = 32;
static_assert(kTailBases + kTailMaxShift == 64, "the reference window of a query is one wavefront");

__device__ __forceinline__ uint64_t tail_key(int32_t tid, int64_t pos, uint32_t side, uint32_t n)
{
    return kKeyedUsed | ((uint64_t)(uint32_t)tid << 39) | ((uint64_t)(uint32_t)pos << 7) | ((uint64_t)side << 6) | n;
}

// the home slot of an entry, and of the query for its (tid, position, side): n stays out of the hash
__device__ __forceinline__ uint64_t tail_home(uint64_t key, int32_t log2_slots) { return keyed_home(key >> 6, log2_slots); }

// per nibble of x (a 4-bit base code each): bit 0 of the nibble set iff the code is one of 1, 2, 4, 8
__device__ __forceinline__ uint32_t nib_one_hot(uint32_t x)
{
    const uint32_t s01 = x | (x >> 1), a01 = x & (x >> 1);
    return (s01 ^ (s01 >> 2)) & ~a01 & ~(a01 >> 2) & 0x11111111u;
}

// bit 0 of each of the 8 nibbles -> bits 0 .. 7
__device__ __forceinline__ uint32_t nib_gather(uint32_t a)
{
    a = (a | (a >> 3)) & 0x03030303u;
    a = (a | (a >> 6)) & 0x000F000Fu;
    return (a | (a >> 12)) & 0xFFu;
}

// The n <= 32 read bases lo .. lo + n - 1 of the packed bases at seq as planes in ASCENDING read order (bit k: base lo + k).
// BAM packs two bases per byte, the earlier one in the HIGH nibble, and lo may be odd: the nibbles of every word are swapped so
// that nibble m of the stream sits at bit 4 m, then the stream moves down by one nibble where lo is odd.  Reads 20 bytes from
// seq + lo / 2, which stay inside the chunk buffer (>= 64 spare bytes behind the last record).  Returns whether all n are A/C/G/T.
__device__ __forceinline__ bool tail_planes(const uint8_t* seq, uint32_t lo, uint32_t n, uint32_t* p_lo, uint32_t* p_hi)
{
    const uint8_t* at = seq + (lo >> 1);
    uint32_t w[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint32_t x = ld_u32(at + 4 * j);
        w[j] = ((x & 0x0F0F0F0Fu) << 4) | ((x >> 4) & 0x0F0F0F0Fu);
    }
    const bool odd = lo & 1u;
    uint32_t lo_plane = 0, hi_plane = 0, ok = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t v = odd ? (w[j] >> 4) | (w[j + 1] << 28) : w[j];
        // codes 1 2 4 8 = A C G T -> 0 1 2 3: the low bit is set for 2 and 8, the high bit for 4 and 8
        lo_plane |= nib_gather(((v >> 1) | (v >> 3)) & 0x11111111u) << (8 * j);
        hi_plane |= nib_gather(((v >> 2) | (v >> 3)) & 0x11111111u) << (8 * j);
        ok |= nib_gather(nib_one_hot(v)) << (8 * j);
    }
    const uint32_t m = n >= 32u ? 0xFFFFFFFFu : (1u << n) - 1u;
    *p_lo = lo_plane & m; *p_hi = hi_plane & m;
    return (ok & m) == m;
}

struct TailScatterArgs {
    im_dev_records recs;
    const int32_t* len;
    int32_t n_contigs;
    int32_t min_clip, min_mapq;
    KeyedTable tab;
};

// what a lane of the scatter has to insert: at most one entry per clipping end
struct TailPair { uint64_t key[2], payload[2]; uint32_t n; };

__device__ __forceinline__ TailPair tail_entries(const TailScatterArgs& A, int64_t i)
{
    TailPair P; P.n = 0; P.key[0] = P.key[1] = P.payload[0] = P.payload[1] = 0;
    if (i >= A.recs.n) return P;
    const uint32_t off = A.recs.rec_off[i], end = A.recs.rec_off[i + 1];
    SpanRec r = span_record(A.recs.raw, off, end);
    const ClipEnds e = clip_decide(r, A.n_contigs, A.min_clip, A.min_mapq);
    if (!e.left && !e.right) return P;                              // ~99 % of the lanes of a 30x chunk end here
    int64_t refend;
    if (!clip_refend(r, e, &refend)) return P;
    const int64_t clen = A.len[r.tid];
    // the packed bases sit behind the CIGAR, with qualities behind them or without: (l_seq + 1) / 2 bytes inside the record
    const int64_t l_seq = (int32_t)ld_u32(r.p + 16);
    const uint32_t o_seq = r.o_cigar + 4u * r.n_cigar;
    if (l_seq <= 0 || (uint64_t)o_seq + (uint64_t)((l_seq + 1) >> 1) > (uint64_t)(end - off)) return P;
    const uint8_t* seq = r.p + o_seq;
    if (e.right && refend >= 0 && refend <= clen && (int64_t)e.len_r <= l_seq) {
        // base i = read base l_seq - L + i: ascending read order is junction order
        const uint32_t n = e.len_r < (uint32_t)kTailBases ? e.len_r : (uint32_t)kTailBases;
        uint32_t pl, ph;
        if (tail_planes(seq, (uint32_t)(l_seq - e.len_r), n, &pl, &ph)) {
            P.key[0] = tail_key(r.tid, refend, 0u, n); P.payload[0] = ((uint64_t)ph << 32) | pl; P.n = 1;
        }
    }
    if (e.left && r.pos >= 0 && r.pos <= clen && (int64_t)e.len_l <= l_seq) {
        // base i = read base L - 1 - i: the bases L - n .. L - 1, reversed
        const uint32_t n = e.len_l < (uint32_t)kTailBases ? e.len_l : (uint32_t)kTailBases;
        uint32_t pl, ph;
        if (tail_planes(seq, e.len_l - n, n, &pl, &ph)) {
            pl = __brev(pl) >> (32u - n); ph = __brev(ph) >> (32u - n);
            const uint64_t key = tail_key(r.tid, r.pos, 1u, n), payload = ((uint64_t)ph << 32) | pl;
            if (P.n == 0u) { P.key[0] = key; P.payload[0] = payload; } else { P.key[1] = key; P.payload[1] = payload; }
            P.n++;
        }
    }
    return P;
}

// one ticket draw per workgroup (keyed_block_tickets has the reason), a lane holding up to two entries
__global__ __launch_bounds__(kTailBlock) void cliptail_scatter_kernel(TailScatterArgs A)
{
    const TailPair P = tail_entries(A, (int64_t)blockIdx.x * kTailBlock + threadIdx.x);
    unsigned long long ticket;
    if (!keyed_block_tickets<kTailBlock, 2>(A.tab, P.n, &ticket)) return;
    const int32_t k = A.tab.log2_slots;
    if (P.n >= 1u && keyed_admit(A.tab, ticket)) keyed_place(A.tab, tail_home(P.key[0], k), P.key[0], P.payload[0]);
    if (P.n == 2u && keyed_admit(A.tab, ticket + 1ull)) keyed_place(A.tab, tail_home(P.key[1], k), P.key[1], P.payload[1]);
}

// for callers that name the events themselves: one lane per entry; positions outside [0, clen] are dropped (no ticket)
__global__ __launch_bounds__(kTailWaveBlock) void cliptail_add_kernel(int32_t n, int32_t tid, int64_t clen, const int32_t* __restrict__ pos,
                                                                 const uint8_t* __restrict__ side, const uint8_t* __restrict__ nbases,
                                                                 const uint32_t* __restrict__ planes, KeyedTable tab)
{
    const int64_t i = (int64_t)blockIdx.x * kTailWaveBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pos[i];
    if (p < 0 || p > clen) return;
    const uint32_t nb = nbases[i], m = nb >= 32u ? 0xFFFFFFFFu : (1u << nb) - 1u;
    const uint64_t key = tail_key(tid, p, side[i], nb);
    keyed_insert(tab, tail_home(key, tab.log2_slots), key, ((uint64_t)(planes[2 * i + 1] & m) << 32) | (planes[2 * i] & m));
}

// the resident reference is upper-cased ASCII: A C G T -> 0 1 2 3, anything else is no base
__device__ __forceinline__ uint32_t ref_code(uint8_t c, bool* valid)
{
    *valid = c == 'A' || c == 'C' || c == 'G' || c == 'T';
    return c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 0u;
}

struct TailWindow { uint64_t lo, hi, ok; };

// lane i names the reference position of the base at distance i from the junction; positions outside [0, clen) are no base
__device__ __forceinline__ TailWindow tail_window(const uint8_t* __restrict__ ref, int64_t clen, int64_t p)
{
    bool valid = false;
    uint32_t code = 0;
    if (p >= 0 && p < clen) code = ref_code(ref[p], &valid);
    TailWindow W;
    W.lo = __ballot(valid && (code & 1u)); W.hi = __ballot(valid && (code & 2u)); W.ok = __ballot(valid);
    return W;
}

// The walk of the probe run of (tid, pos, side), whatever the entries' n: keyed_walk has each(has, key, slot).  Returns the entries
// stored at the key (wave-uniform); a position outside [0, clen] has none.
template <class Each>
__device__ __forceinline__ uint32_t tail_walk(const KeyedTable& T, int32_t tid, int64_t pos, uint32_t side, int64_t clen, int lane, Each each)
{
    if (pos < 0 || pos > clen) return 0;
    const uint64_t want = tail_key(tid, pos, side, 0u) >> 6;
    return keyed_walk(T, tail_home(want << 6, T.log2_slots), [want](uint64_t key) { return (key >> 6) == want; }, lane, each);
}

// The shift-compare of one batch.  A lane whose slot holds an entry of the key (has; key: n in its low bits, payload: the two planes)
// tests the shifts 0 .. S against the window: a shift of the planes, two XORs, the window's validity, a mask of n bits and a
// popcount.  Returns what lane s adds to v(s) from the ballots.
__device__ __forceinline__ uint32_t tail_shifts(bool has, uint64_t key, uint64_t payload, const TailWindow& W, int32_t S, int lane)
{
    uint32_t mine = 0;
    const uint32_t e_lo = (uint32_t)payload, e_hi = (uint32_t)(payload >> 32);
    const uint32_t n = (uint32_t)key & 63u, m = n >= 32u ? 0xFFFFFFFFu : (1u << n) - 1u, allowed = n >> 4;
    for (int32_t sh = 0; sh <= S; sh++) {                           // wave-uniform
        const uint32_t diff = (((uint32_t)(W.lo >> sh) ^ e_lo) | ((uint32_t)(W.hi >> sh) ^ e_hi) | ~(uint32_t)(W.ok >> sh)) & m;
        const uint64_t match = __ballot(has && (uint32_t)__builtin_popcount(diff) <= allowed);
        if (lane == sh) mine += (uint32_t)__builtin_popcountll(match);
    }
    return mine;
}

// One side of a verify query: the walk, and the shift-compare of every batch that holds entries of the key.  Lane s gathers v(s).
// Returns the entries stored at the key (wave-uniform); *v: this lane's v(lane).
__device__ __forceinline__ uint32_t tail_side(const KeyedTable& T, int32_t tid, int64_t pos, uint32_t side, int64_t clen, const TailWindow& W,
                                              bool compare, int32_t S, int lane, uint32_t* v)
{
    uint32_t mine = 0;
    const uint32_t stored = tail_walk(T, tid, pos, side, clen, lane, [&](bool has, uint64_t key, uint64_t s) {
        if (!compare) return;
        mine += tail_shifts(has, key, has ? T.slots[2ull * s + 1ull] : 0ull, W, S, lane);
    });
    *v = mine;
    return stored;
}

// The chosen shift of a query: the largest vR(s) + vL(s) over s = 0 .. S, the smallest s among equals (the wave's maximum over
// sum : ~s).  vr, vl: this lane's v(lane).  Returns whether any entry matched at any shift; *best, *br, *bl: wave-uniform.
__device__ __forceinline__ bool tail_best_shift(uint32_t vr, uint32_t vl, int32_t S, int lane, int* best, uint32_t* br, uint32_t* bl)
{
    uint64_t key = ((uint64_t)(lane <= S ? vr + vl : 0u) << 32) | (0xFFFFFFFFu - (uint32_t)lane);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(key >> 32), o), lo = (uint32_t)__shfl_xor((int)(uint32_t)key, o);
        const uint64_t k = ((uint64_t)hi << 32) | lo;
        key = k > key ? k : key;
    }
    const bool found = (key >> 32) != 0ull;
    *best = found ? (int)(0xFFFFFFFFu - (uint32_t)key) : 0;
    *br = (uint32_t)__shfl((int)vr, *best); *bl = (uint32_t)__shfl((int)vl, *best);
    return found;
}

// The window the entries of a pile on `side` are expected to hold, given the other pile at position o: right entries (side 0) read on
// from o, left entries (side 1) read backwards from o - 1; across an inversion's junction the directions swap and the bases are the
// other strand's.  The complement of A 0, C 1, G 2, T 3 is both planes inverted; what is no base stays no base.
__device__ __forceinline__ TailWindow tail_expected_window(const uint8_t* __restrict__ ref, int64_t clen, int64_t o, uint32_t side, bool inverted, int lane)
{
    const bool forward = (side == 0u) != inverted;
    TailWindow W = tail_window(ref, clen, forward ? o + lane : o - 1 - lane);
    if (inverted) { W.lo = ~W.lo; W.hi = ~W.hi; }
    return W;
}

// A pile fetched once for many comparisons: when one batch of the walk shows all holders (the usual pile of tens of reads) its
// entries stay in the lanes, and a comparison costs no walk; a pile spread over several batches is walked per comparison.
struct TailHeld { int batches; bool has; uint64_t key, payload; uint32_t stored; };

__device__ __forceinline__ TailHeld tail_hold(const KeyedTable& T, int32_t tid, int64_t pos, uint32_t side, int64_t clen, int lane)
{
    TailHeld H; H.batches = 0; H.has = false; H.key = 0; H.payload = 0;
    H.stored = tail_walk(T, tid, pos, side, clen, lane, [&](bool has, uint64_t key, uint64_t s) {
        if (H.batches++ == 0) { H.has = has; H.key = key; H.payload = has ? T.slots[2ull * s + 1ull] : 0ull; }
    });
    return H;
}

// this lane's v(lane) of the held pile against the window W
__device__ __forceinline__ uint32_t tail_held_shifts(const TailHeld& H, const KeyedTable& T, int32_t tid, int64_t pos, uint32_t side, int64_t clen,
                                                     const TailWindow& W, int32_t S, int lane)
{
    if (H.batches <= 1) return tail_shifts(H.has, H.key, H.payload, W, S, lane);
    uint32_t v;
    (void)tail_side(T, tid, pos, side, clen, W, true, S, lane, &v);
    return v;
}

struct TailVerifyArgs {
    int32_t nq, tid, max_shift;
    const int32_t* pr;
    const int32_t* pl;
    const uint8_t* ref;         // the contig's ASCII bases
    int64_t clen;
    KeyedTable tab;
    uint32_t* v_right;
    uint32_t* v_left;
    int32_t* shift;
    uint32_t* stored_right;
    uint32_t* stored_left;
};

// One wave per query (pr: where right clips pile up, pl: where left clips do).  A right entry at pr continues at pl + s, a left entry
// at pl continues backwards from pr - 1 - s: one 64-base window per side, fetched once.  The chosen shift: tail_best_shift.
__global__ __launch_bounds__(kTailWaveBlock) void cliptail_verify_kernel(TailVerifyArgs A)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < A.nq; q += nwaves) {
        const int64_t pr = A.pr[q], pl = A.pl[q];
        const bool compare = pl > pr;
        const TailWindow Wr = tail_expected_window(A.ref, A.clen, pl, 0u, false, lane);
        const TailWindow Wl = tail_expected_window(A.ref, A.clen, pr, 1u, false, lane);
        uint32_t vr, vl;
        const uint32_t sr = tail_side(A.tab, A.tid, pr, 0u, A.clen, Wr, compare, A.max_shift, lane, &vr);
        const uint32_t sl = tail_side(A.tab, A.tid, pl, 1u, A.clen, Wl, compare, A.max_shift, lane, &vl);
        int best;
        uint32_t br, bl;
        const bool found = tail_best_shift(vr, vl, A.max_shift, lane, &best, &br, &bl);
        if (lane == 0) {
            A.v_right[q] = found ? br : 0u; A.v_left[q] = found ? bl : 0u; A.shift[q] = found ? best : -1;
            A.stored_right[q] = sr; A.stored_left[q] = sl;
        }
    }
}

// Junctions (include/indelminer_amd.h, seam 5, "Junctions"): one wave per query (tid1, p1, side1, tid2, p2, side2), the two ends on
// contigs of their own or on one, in any order.  The entries of an end are expected to hold the OTHER end's contig: forwards from its
// position when that end's pile is of left clips, backwards from the base in front of it when it is of right clips, the other strand
// when the two sides are equal -- tail_expected_window with the other contig's bases and length, one 64-base window per end, fetched
// once.  The chosen shift: tail_best_shift.  The contigs' offsets are 64-bit, as everywhere.
__global__ __launch_bounds__(kTailWaveBlock) void cliptail_junction_kernel(TailJunctionArgs A)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < A.nq; q += nwaves) {
        const int32_t t1 = A.tid1[q], t2 = A.tid2[q];
        const int64_t p1 = A.p1[q], p2 = A.p2[q];
        const uint32_t s1 = A.side1[q], s2 = A.side2[q];
        const int64_t clen1 = A.ref.len[t1], clen2 = A.ref.len[t2];
        const uint8_t* __restrict__ ref1 = A.ref.ascii + A.ref.asc_off[t1];
        const uint8_t* __restrict__ ref2 = A.ref.ascii + A.ref.asc_off[t2];
        const bool inverted = s1 == s2;
        const TailWindow W1 = tail_expected_window(ref2, clen2, p2, s1, inverted, lane);
        const TailWindow W2 = tail_expected_window(ref1, clen1, p1, s2, inverted, lane);
        uint32_t v1, v2;
        const uint32_t st1 = tail_side(A.tab, t1, p1, s1, clen1, W1, true, A.max_shift, lane, &v1);
        const uint32_t st2 = tail_side(A.tab, t2, p2, s2, clen2, W2, true, A.max_shift, lane, &v2);
        int best;
        uint32_t b1, b2;
        const bool found = tail_best_shift(v1, v2, A.max_shift, lane, &best, &b1, &b2);
        if (lane == 0) {
            A.v1[q] = found ? b1 : 0u; A.v2[q] = found ? b2 : 0u; A.shift[q] = found ? best : -1;
            A.stored1[q] = st1; A.stored2[q] = st2;
        }
    }
}

// the first index of the ascending list at which pos[i] >= x (n when there is none): every lane runs the same search
__device__ __forceinline__ int32_t first_at_or_behind(const int32_t* __restrict__ pos, int32_t n, int64_t x)
{
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)pos[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Pairs of piles (include/indelminer_amd.h, seam 5, "Crossed piles" and "Inverted piles"): ONE BODY, two geometries.
//                 the wave's peak p, pile side s       its partners o, pile side t                              windows
//   crossed  (-U) a peak of the right list, s = 0      the LEFT list inside [p - max_len, p - min_len], t = 1   this strand
//   inverted (-N) a peak of either list, s = its side  the SAME list inside [p + min_len, p + max_len], t = s   the other strand
// (the inverted waves below n_right take the right peaks, the others the left ones).  The partners are a run of a sorted list, found by
// two binary searches; a peak without one ends there.  What depends on p alone is fetched once: the window the entries of every
// partner are expected to hold (tail_expected_window of p for side t), and the pile at p (tail_hold: in the lanes when one batch of
// the walk holds it all, walked per partner otherwise).  Per partner: the window the held entries are expected to hold and v1(.) of
// the held pile; ONLY when some shift has v1 >= min_verified the walk of the pile at o for v2(.), the chosen shift, the
// qualification.  That first cut changes no answer -- a pair qualifies only with v1 >= min_verified at the chosen shift, so a held
// pile that reaches it at no shift has no pair here -- and a chance pair of peaks so costs one 64-byte load and one shift loop.  The
// rare pair that qualifies takes its slot with one returning atomic by lane 0; n_found counts every pair, only slots below cap are
// written, column k at col[k][slot]: side (0 for crossed), p1 = p, p2 = o, their counts, v1, v2, shift, stored at p,
// stored at o.  Every branch is on values the whole wave shares; kInverted is a compile-time parameter so that neither instantiation
// carries the other's selects.
template <bool kInverted>
__global__ __launch_bounds__(kTailWaveBlock) void cliptail_pairs_kernel(TailPairsArgs A)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    const int n_all = kInverted ? A.n_right + A.n_left : A.n_right;
    for (int q = wave; q < n_all; q += nwaves) {
        const bool left = kInverted && q >= A.n_right;
        const bool pleft = kInverted ? left : true;                 // the partners' list
        const uint32_t side = left ? 1u : 0u, pside = pleft ? 1u : 0u;
        const int32_t* __restrict__ pos = left ? A.lpos : A.rpos;
        const uint32_t* __restrict__ cnt = left ? A.lcnt : A.rcnt;
        const int32_t* __restrict__ ppos = pleft ? A.lpos : A.rpos;
        const uint32_t* __restrict__ pcnt = pleft ? A.lcnt : A.rcnt;
        const int32_t pn = pleft ? A.n_left : A.n_right, at = left ? q - A.n_right : q;
        const int64_t p = pos[at];
        const int32_t k0 = first_at_or_behind(ppos, pn, kInverted ? p + (int64_t)A.min_len : p - (int64_t)A.max_len);
        const int32_t k1 = first_at_or_behind(ppos, pn, (kInverted ? p + (int64_t)A.max_len : p - (int64_t)A.min_len) + 1);
        if (k0 >= k1) continue;
        const TailWindow Wp = tail_expected_window(A.ref, A.clen, p, pside, kInverted, lane);
        const TailHeld H = tail_hold(A.tab, A.tid, p, side, A.clen, lane);
        for (int32_t k = k0; k < k1; k++) {
            const int64_t o = ppos[k];
            const TailWindow Wo = tail_expected_window(A.ref, A.clen, o, side, kInverted, lane);
            const uint32_t v1 = tail_held_shifts(H, A.tab, A.tid, p, side, A.clen, Wo, A.max_shift, lane);
            if (!__ballot(lane <= A.max_shift && v1 >= (uint32_t)A.min_verified)) continue;     // the first cut: no trip to the table
            uint32_t v2;
            const uint32_t s2 = tail_side(A.tab, A.tid, o, pside, A.clen, Wp, true, A.max_shift, lane, &v2);
            int best;
            uint32_t b1, b2;
            const bool found = tail_best_shift(v1, v2, A.max_shift, lane, &best, &b1, &b2);
            if (!found || b1 < (uint32_t)A.min_verified || b2 < (uint32_t)A.min_verified) continue;
            if (lane == 0) {
                const uint32_t slot = atomicAdd(A.n_found, 1u);
                if (slot < (uint32_t)A.cap) {
                    A.col[0][slot] = side; A.col[1][slot] = (uint32_t)p; A.col[2][slot] = (uint32_t)o; A.col[3][slot] = cnt[at]; A.col[4][slot] = pcnt[k];
                    A.col[5][slot] = b1; A.col[6][slot] = b2; A.col[7][slot] = (uint32_t)best; A.col[8][slot] = H.stored; A.col[9][slot] = s2;
                }
            }
        }
    }
}

struct TailConsensusArgs {
    int32_t nq, tid, min_cover;
    const int32_t* pos;
    const uint8_t* side;
    int64_t clen;
    KeyedTable tab;
    uint32_t* entries;
    uint32_t* len;
    uint32_t* planes;           // two per query: low bits, high bits
    uint32_t* agree;
};

// One wave per query (tid, pos, side): the per-base consensus of the entries stored at the key (-I).  First walk: for base
// i = 0 .. 31 (wave-uniform) three ballots over the lanes that hold an entry with n > i -- those, their low bits, their high bits --
// give the four codes' counts at i as popcounts, and lane i keeps them.  Lanes 0 .. 31 then pick their base (the most entries, the
// smallest code among equals) where cover(i) >= min_cover; cover does not increase with i, so those lanes are 0 .. len - 1 and two
// ballots give the planes.  Second walk: the entries that differ from the consensus in at most min(n, len) >> 4 of their first
// min(n, len) bases.  Counts are sums over the entries: nothing depends on the order they arrived in.
__global__ __launch_bounds__(kTailWaveBlock) void cliptail_consensus_kernel(TailConsensusArgs A)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < A.nq; q += nwaves) {
        const int64_t pos = A.pos[q];
        const uint32_t side = A.side[q];
        uint32_t cnt[4] = {0u, 0u, 0u, 0u};
        const uint32_t stored = tail_walk(A.tab, A.tid, pos, side, A.clen, lane, [&](bool has, uint64_t key, uint64_t s) {
            const uint64_t payload = has ? A.tab.slots[2ull * s + 1ull] : 0ull;
            const uint32_t e_lo = (uint32_t)payload, e_hi = (uint32_t)(payload >> 32);
            const uint32_t n = has ? (uint32_t)key & 63u : 0u;
#pragma unroll 4
            for (int i = 0; i < kTailBases; i++) {                  // wave-uniform
                const uint64_t cov = __ballot(n > (uint32_t)i);
                const uint64_t lo = __ballot(n > (uint32_t)i && ((e_lo >> i) & 1u)), hi = __ballot(n > (uint32_t)i && ((e_hi >> i) & 1u));
                if (lane == i) {
                    cnt[0] += (uint32_t)__builtin_popcountll(cov & ~lo & ~hi); cnt[1] += (uint32_t)__builtin_popcountll(lo & ~hi);
                    cnt[2] += (uint32_t)__builtin_popcountll(hi & ~lo); cnt[3] += (uint32_t)__builtin_popcountll(lo & hi);
                }
            }
        });
        const bool covered = lane < kTailBases && cnt[0] + cnt[1] + cnt[2] + cnt[3] >= (uint32_t)A.min_cover;
        uint32_t code = 0, most = cnt[0];
#pragma unroll
        for (uint32_t c = 1; c < 4u; c++) if (cnt[c] > most) { most = cnt[c]; code = c; }      // strictly: the smallest code among equals stays
        const uint32_t len = (uint32_t)__builtin_popcountll(__ballot(covered));
        const uint32_t c_lo = (uint32_t)__ballot(covered && (code & 1u)), c_hi = (uint32_t)__ballot(covered && (code & 2u));
        uint32_t agree = 0;
        if (len > 0u) {
            (void)tail_walk(A.tab, A.tid, pos, side, A.clen, lane, [&](bool has, uint64_t key, uint64_t s) {
                const uint64_t payload = has ? A.tab.slots[2ull * s + 1ull] : 0ull;
                const uint32_t n = (uint32_t)key & 63u, k = n < len ? n : len, m = k >= 32u ? 0xFFFFFFFFu : (1u << k) - 1u;
                const uint32_t diff = (((uint32_t)payload ^ c_lo) | ((uint32_t)(payload >> 32) ^ c_hi)) & m;
                agree += (uint32_t)__builtin_popcountll(__ballot(has && (uint32_t)__builtin_popcount(diff) <= (k >> 4)));
            });
        }
        if (lane == 0) { A.entries[q] = stored; A.len[q] = len; A.planes[2 * q] = c_lo; A.planes[2 * q + 1] = c_hi; A.agree[q] = agree; }
    }
}

}  // namespace

hipError_t launch_cliptail_consensus(int32_t nq, int32_t tid, const int32_t* pos, const uint8_t* side, int32_t min_cover, int64_t clen,
                                     const KeyedTable& tab, uint32_t* entries, uint32_t* len, uint32_t* planes, uint32_t* agree, hipStream_t stream)
{
    if (nq <= 0) return hipSuccess;
    TailConsensusArgs A;
    A.nq = nq; A.tid = tid; A.min_cover = min_cover; A.pos = pos; A.side = side; A.clen = clen; A.tab = tab;
    A.entries = entries; A.len = len; A.planes = planes; A.agree = agree;
    hipLaunchKernelGGL(cliptail_consensus_kernel, dim3(wave_grid(nq)), dim3(kTailWaveBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_cliptail_pairs(bool inverted, TailPairsArgs A, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(A.n_found, 0, sizeof(uint32_t), stream);
    if (A.n_right < 0) A.n_right = 0;
    if (A.n_left < 0) A.n_left = 0;
    // crossed: a wave per right peak, and nothing to pair it with while the left list is empty; inverted: a wave per peak of either list
    const int64_t waves = inverted ? (int64_t)A.n_right + A.n_left : A.n_left > 0 ? A.n_right : 0;
    if (e != hipSuccess || waves == 0) return e;
    if (inverted) hipLaunchKernelGGL(cliptail_pairs_kernel<true>, dim3(wave_grid(waves)), dim3(kTailWaveBlock), 0, stream, A);
    else hipLaunchKernelGGL(cliptail_pairs_kernel<false>, dim3(wave_grid(waves)), dim3(kTailWaveBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_cliptail_scatter(const RefDev& ref, int32_t min_clip, int32_t min_mapq, const im_dev_records& recs, const KeyedTable& tab,
                                   hipStream_t stream)
{
    if (recs.n <= 0) return hipSuccess;
    TailScatterArgs A;
    A.recs = recs; A.len = ref.len; A.n_contigs = ref.n_contigs; A.min_clip = min_clip; A.min_mapq = min_mapq; A.tab = tab;
    hipLaunchKernelGGL(cliptail_scatter_kernel, dim3((recs.n + kTailBlock - 1) / kTailBlock), dim3(kTailBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_cliptail_add(int32_t n, int32_t tid, int64_t clen, const int32_t* pos, const uint8_t* side, const uint8_t* nbases,
                               const uint32_t* planes, const KeyedTable& tab, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(cliptail_add_kernel, dim3((n + kTailWaveBlock - 1) / kTailWaveBlock), dim3(kTailWaveBlock), 0, stream, n, tid, clen, pos, side, nbases, planes, tab);
    return hipGetLastError();
}

hipError_t launch_cliptail_verify(int32_t nq, int32_t tid, const int32_t* pr, const int32_t* pl, int32_t max_shift, const uint8_t* ref,
                                  int64_t clen, const KeyedTable& tab, uint32_t* v_right, uint32_t* v_left, int32_t* shift,
                                  uint32_t* stored_right, uint32_t* stored_left, hipStream_t stream)
{
    if (nq <= 0) return hipSuccess;
    TailVerifyArgs A;
    A.nq = nq; A.tid = tid; A.max_shift = max_shift; A.pr = pr; A.pl = pl; A.ref = ref; A.clen = clen; A.tab = tab;
    A.v_right = v_right; A.v_left = v_left; A.shift = shift; A.stored_right = stored_right; A.stored_left = stored_left;
    hipLaunchKernelGGL(cliptail_verify_kernel, dim3(wave_grid(nq)), dim3(kTailWaveBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_cliptail_junction(const TailJunctionArgs& A, hipStream_t stream)
{
    if (A.nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(cliptail_junction_kernel, dim3(wave_grid(A.nq)), dim3(kTailWaveBlock), 0, stream, A);
    return hipGetLastError();
}

}  // namespace im
