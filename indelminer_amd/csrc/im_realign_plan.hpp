// im_realign_plan.hpp -- the control skeleton of split-read realignment, shared by every realign kernel (device only).
//
// attempt_pe_alignment / attempt_diagonal_alignments (src/alignment.c:535-799) and update_readsegs (src/readaln.c:348-458)
// around the band searches and the dynamic programs, which stay with the kernels (im_realign.hip, im_realign_long.hip,
// im_realign_any.hip):
//
//   realign_windows   the two windows around the anchor and their validity          774-783, 548-553
//   plan_piece2       the four-case plan for the second piece                       605-717
//   accept_piece2     whether the second alignment is one the merge can use         623-627, 645-649, 679-683, 701-705, 720-721
//   choose_pieces     which piece is A (starts at read offset 0) / B (ends at L)    723-754
//   merge_pieces<PPL> the wave-cooperative merge of two GAPLESS pieces              K4 219-339, readaln.c:348-458, evidence.c:4-34
//
// The first four are plain scalar code: the one-wave-per-read kernels hand them wave-uniform values (SGPRs, scalar
// branches), realign_any_kernel runs them per lane.  merge_pieces is wave-cooperative (PPL read positions per lane) and
// serves the two numgaps == 0 kernels only; pieces with inner I / D ops go through band_build_result / any_build_result.
// No function here carries a phase stamp (IM_STAMP): those sit at the call sites.
#pragma once

#include "im_device.hpp"
#include "im_wave.hpp"

namespace im {
namespace {

constexpr int kStGoOn = -100;           // "no verdict yet, go on": not an IM_ST_* value

// window geometry (src/alignment.c:774-783) and attempt_diagonal_alignments' entry check (548-553)
struct Windows { int left1, right1, left2, right2; bool ok; };

__device__ __forceinline__ Windows realign_windows(int anchor, int R, uint32_t maxdelsize, int clen)
{
    Windows w;
    int distance = R;
    w.left1  = anchor >= distance ? anchor - distance : 0;
    w.right1 = clen < (anchor + distance) ? clen : anchor + distance;
    distance = R + (int)maxdelsize;
    w.left2  = anchor >= distance ? anchor - distance : 0;
    w.right2 = clen < (anchor + distance) ? clen : anchor + distance;
    w.ok = anchor >= w.left1 && anchor >= w.left2 && anchor <= w.right1 && anchor <= w.right2 &&
           w.left2 >= 0 && w.right2 > 0;                                                            // 548-553
    return w;
}

// Piece 2: the rest of the read in the extended window, four cases (605-717).  [r1,r2) x [q1,q2) is the
// first alignment, f / l its leading / trailing '=' runs (585-599); the guards in unsigned arithmetic as written.
// st: kStGoOn with the second search's window [w0,w1), anchor, read piece [p0,p1) and which end of the read the second
// alignment has to reach; IM_ST_ABORT where the reference's forceassert(L > f) fires (tested before the flanks of its
// branch); IM_ST_NONE where a flank is below the evidence threshold or the geometry has no case.
struct Piece2Plan { int st; uint32_t w0, w1, anc, p0, p1; bool want_tail; };

__device__ __forceinline__ Piece2Plan plan_piece2(int r1, int r2, int q1, int q2, uint32_t f, uint32_t l, int L, int anchor,
                                                  int left2, int right2, uint32_t eth)
{
    Piece2Plan p;
    p.st = IM_ST_NONE; p.w0 = p.w1 = p.anc = p.p0 = p.p1 = 0u; p.want_tail = false;
    const uint32_t uL = (uint32_t)L;
    if (r1 > anchor) {
        if (q1 == 0) {
            if (!(uL > f)) { p.st = IM_ST_ABORT; return p; }
            if ((uL - f) < eth || ((uint32_t)right2 - (uint32_t)r1 - f) < eth) return p;
            p.w0 = (uint32_t)r1 + f; p.w1 = (uint32_t)right2; p.anc = (uint32_t)r1; p.p0 = f; p.p1 = uL; p.want_tail = true;
        } else if (q2 == L) {
            if (!(uL > l)) { p.st = IM_ST_ABORT; return p; }
            if ((uL - l) < eth || ((uint32_t)r2 - l - (uint32_t)anchor) < eth) return p;
            p.w0 = (uint32_t)anchor; p.w1 = (uint32_t)r2 - l; p.anc = (uint32_t)r2; p.p0 = 0; p.p1 = uL - l; p.want_tail = false;
        } else return p;
    } else if (r1 < anchor) {
        if (r2 >= anchor) return p;
        if (q1 == 0) {
            if (!(uL > f)) { p.st = IM_ST_ABORT; return p; }
            if ((uL - f) < eth || ((uint32_t)anchor - (uint32_t)r1 - f) < eth) return p;
            p.w0 = (uint32_t)r1 + f; p.w1 = (uint32_t)anchor; p.anc = (uint32_t)r1; p.p0 = f; p.p1 = uL; p.want_tail = true;
        } else if (q2 == L) {
            if (!(uL > l)) { p.st = IM_ST_ABORT; return p; }
            if ((uL - l) < eth || ((uint32_t)r2 - l - (uint32_t)left2) < eth) return p;
            p.w0 = (uint32_t)left2; p.w1 = (uint32_t)r2 - l; p.anc = (uint32_t)r2; p.p0 = 0; p.p1 = uL - l; p.want_tail = false;
        } else return p;
    } else return p;                                                                                // r1 == anchor (712-717)
    p.st = ((int32_t)(p.w1 - p.w0) <= 0) ? IM_ST_ABORT : kStGoOn;
    return p;
}

// The second alignment [q3,q4) must reach the end of the read the plan asked for, and not be empty: IM_ST_NONE otherwise
// (623-627, 679-683 / 645-649, 701-705).  IM_ST_ABORT: forceassert((q1 < q2) && (q3 < q4)), 720-721.
__device__ __forceinline__ int accept_piece2(bool want_tail, int q1, int q2, int q3, int q4, int L)
{
    if (want_tail) { if (q4 != L || q3 == q4) return IM_ST_NONE; }
    else           { if (q3 != 0 || q3 == q4) return IM_ST_NONE; }
    if (!(q1 < q2 && q3 < q4)) return IM_ST_ABORT;
    return kStGoOn;
}

// combine (723-754).  "A" = the piece that starts at read offset 0, "B" = the one that ends at L: A = read[.,qa2) at contig
// rA.., B = read[qb1,.) at contig rB...  a_is_second: A is the second alignment (q3, q4, r3, r4), B the first.
// split: the pieces overlap in the read, the split point is to be chosen (K4, find_best_del_candidate); otherwise they
// meet on the reference with read bases between them.  !ok: no case applies (IM_ST_NONE).
struct Pieces { bool ok, a_is_second, split; int qa2, rA, qb1, rB; };

__device__ __forceinline__ Pieces choose_pieces(int q1, int q2, int q3, int q4, int r1, int r2, int r3, int r4)
{
    Pieces p;
    p.ok = true;
    if (q1 > q3 && q1 <= q4)        { p.a_is_second = true;  p.split = true;  }                     // 724-731
    else if (q3 > q1 && q3 <= q2)   { p.a_is_second = false; p.split = true;  }                     // 732-739
    else if (q1 > q4 && r1 == r4)   { p.a_is_second = true;  p.split = false; }                     // 740-744
    else if (q3 > q2 && r2 == r3)   { p.a_is_second = false; p.split = false; }                     // 745-749
    else                            { p.a_is_second = false; p.split = false; p.ok = false; }
    p.qa2 = p.a_is_second ? q4 : q2; p.rA = p.a_is_second ? r3 : r1;
    p.qb1 = p.a_is_second ? q1 : q3; p.rB = p.a_is_second ? r1 : r3;
    return p;
}

// The merge of two gapless pieces by the whole wave, lane l owning the PPL read positions PPL l .. PPL l + PPL - 1:
// the split point (find_best_del_candidate / count_matches, src/alignment.c:219-339), update_readsegs
// (src/readaln.c:348-458) in closed form, the one evidence record (new_evidence, src/evidence.c:4-34) and the read's
// evidence slots.  eqA / eqB: bit j set where this lane's position j is an aligned '=' of A / B (bits outside the
// pieces are ignored: A counts on [0,qa2), B on [qb1,L)).  bpos: IM_MAX_OPS + 1 ints of LDS nobody else uses meanwhile.
// Returns IM_ST_EVIDENCE with the record complete, or the status the caller finishes the read with.
// PPL <= 4 means L <= 255 (kShortRead; PPL == 2: L <= 128): both prefix counts then travel in one scan and the split
// search is one packed maximum -- realign_kernel is bound by instruction issue and keeps both.
template <int PPL>
__device__ __forceinline__ int merge_pieces(uint32_t eqA, uint32_t eqB, int qa2, int rA, int qb1, int rB, bool split, int L,
                                            int32_t* bpos, im_read_result* out, const RealignArgs& A, int c, int lane)
{
    static_assert(PPL == 2 || PPL == 4 || PPL == 16, "two positions per lane (reads up to 128 bases), four (up to kShortRead) or sixteen");
    // per-position match flags of A on [0,qa2) and B on [qb1,L)
    const int x0 = PPL * lane;
    uint32_t fa = 0, fb = 0;
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        const int x = x0 + j;
        fa |= (x < qa2) ? (eqA & (1u << j)) : 0u;
        fb |= (x >= qb1 && x < L) ? (eqB & (1u << j)) : 0u;
    }
    const int ta = __popc(fa), tb = __popc(fb);
    int ia, ib, totA, totB;
    if constexpr (PPL <= 4) {
        const int iab = wave_scan_add(ta | (tb << 16), lane);          // both counts in one scan: each stays below 2^15
        const int tot = __builtin_amdgcn_readlane(iab, 63);
        ia = iab & 0xFFFF; ib = iab >> 16;
        totA = tot & 0xFFFF; totB = tot >> 16;
    } else {
        ia = wave_scan_add(ta, lane); ib = wave_scan_add(tb, lane);
        totA = __builtin_amdgcn_readlane(ia, 63); totB = __builtin_amdgcn_readlane(ib, 63);
    }
    const int ea0 = ia - ta, eb0 = ib - tb;             // '=' of A / B in front of x0

    int index, nextindex, matches;
    if (split) {
        // count_matches(i) = '=' of A in read[0,i) + '=' of B in read[i,L); X counts are L - that, so "max matches,
        // then min mismatches, first wins" is the first maximum.
        if constexpr (PPL <= 4) {
            // one reduction for both: (matches << 8) | (255 - x), largest wins -- matches and x stay below 256
            int bk = -1;
#pragma unroll
            for (int j = 0; j < PPL; j++) {
                const int x = x0 + j;
                const uint32_t below = (1u << j) - 1u;
                const int sc = ea0 + __popc(fa & below) + (totB - eb0 - __popc(fb & below));
                if (x >= qb1 && x <= qa2) bk = max(bk, (sc << 8) | (255 - x));
            }
            bk = wave_max(bk);
            if (bk < 0) return IM_ST_ABORT;                                                 // forceassert(index != -1)
            index = 255 - (bk & 255);
            matches = bk >> 8;
        } else {
            int bs = -1, bx = INT_MAX;
#pragma unroll
            for (int j = 0; j < PPL; j++) {
                const int x = x0 + j;
                if (x >= qb1 && x <= qa2) {
                    const uint32_t below = (1u << j) - 1u;
                    const int sc = ea0 + __popc(fa & below) + (totB - eb0 - __popc(fb & below));
                    if (sc > bs) { bs = sc; bx = x; }
                }
            }
            const int best = wave_max(bs);
            index = wave_min(bs == best ? bx : INT_MAX);
            if (best < 0 || index == INT_MAX) return IM_ST_ABORT;                           // forceassert(index != -1)
            matches = best;
        }
        nextindex = index;
    } else {
        index = qa2; nextindex = qb1;
        matches = totA + totB;
    }

    // update_readsegs (src/readaln.c:348-458) in closed form: A's runs over [0,index), an I of nextindex-index bases if
    // the pieces leave read bases uncovered, a D if the reference positions leave a gap, then B's runs over [nextindex,L).
    const int refindx = rA + index;
    const int rindex  = rB + (nextindex - qb1);
    const bool hasI = nextindex > index;
    const bool hasD = refindx < rindex;
    if (!hasI && !hasD) return IM_ST_NONE;                                                  // no D/I segment -> NULL

    // run-length encode the final per-position classes
    int cls[PPL];
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        const int x = x0 + j;
        cls[j] = (x >= L) ? -1 : (x < index) ? (((fa >> j) & 1u) ? IM_OP_EQ : IM_OP_X)
                 : (x < nextindex) ? IM_OP_I : (((fb >> j) & 1u) ? IM_OP_EQ : IM_OP_X);
    }
    const int prevc = dpp_mov<kDppWaveShr1>(-2, cls[PPL - 1]);      // lane 0 keeps -2
    uint32_t bnd = 0;
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        const int x = x0 + j;
        const int pc = (j == 0) ? prevc : cls[j - 1];
        if ((x < L) && (x == 0 || x == index || x == nextindex || cls[j] != pc)) bnd |= 1u << j;
    }
    const int nb = __popc(bnd);
    const int inb = wave_scan_add(nb, lane);
    const int total_b = __builtin_amdgcn_readlane(inb, 63);
    const int n_ops = total_b + (hasD ? 1 : 0);
    // this bound is also what keeps the bpos[] writes below inside the caller's IM_MAX_OPS + 1 ints: it must stay in front of them
    if (n_ops > IM_MAX_OPS) return IM_ST_OVERFLOW;
    // run length = distance to the next boundary: boundary k leaves its position in LDS, run k ends where boundary k+1 starts
    {
        int k = inb - nb;
#pragma unroll
        for (int j = 0; j < PPL; j++) if ((bnd >> j) & 1u) bpos[k++] = x0 + j;
        if (lane == 0) bpos[total_b] = L;
    }
    wave_lds_sync();
    int slot = inb - nb;                 // boundaries before this lane
    int seg_indel = 0;
#pragma unroll
    for (int j = 0; j < PPL; j++) {
        const int x = x0 + j;
        if ((bnd >> j) & 1u) {
            const int sl = slot + ((hasD && x >= nextindex) ? 1 : 0);
            out->ops[sl] = ((uint32_t)(bpos[slot + 1] - x) << 4) | (uint32_t)cls[j];
            if (x == index) seg_indel = slot;       // the I run itself, or the run the D op goes in front of
            slot++;
        }
    }
    // the lane that owns read position `index` set it (0 if index == L: no lane owns L -- at PPL == 2 and L == 128 that is
    // lane 64, which is lane 0 again, and lane 0 owns no boundary at `index` then)
    seg_indel = __builtin_amdgcn_readlane(seg_indel, ((uint32_t)index / PPL) & 63u);
    if (lane == 0) {
        if (hasD) out->ops[seg_indel] = ((uint32_t)(rindex - refindx) << 4) | IM_OP_D;
        im_evidence* e = &out->ev[0];
        e->cls = hasD ? IM_CLS_DELETION : IM_CLS_INSERTION;
        e->b1 = refindx; e->b2 = hasD ? rindex : refindx;
        e->lflank = index; e->rflank = L - nextindex;
        e->seg = seg_indel;
        e->read_off = index;
        // X bases left in aln1 + aln3: aligned bases minus '=' bases
        const int aligned = index + (L - nextindex);
        e->nd_print = aligned - matches;
        e->nd_filter = aligned - matches;
        out->ref_start = rA;
        out->n_ops = n_ops;
        out->n_ev = 1;
        out->status = IM_ST_EVIDENCE;
        out->n_band = 2;
    }
    write_slots(A, c, 1, hasD ? IM_CLS_DELETION : IM_CLS_INSERTION, refindx, hasD ? rindex : refindx, lane);
    return IM_ST_EVIDENCE;
}

}  // namespace
}  // namespace im
