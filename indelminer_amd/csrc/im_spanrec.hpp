// im_spanrec.hpp -- what the scatter kernels read of a delivered record's core and CIGAR, and the clip decision of -C.  Device code
// only; used by im_span.hip (span, pair and clip scatter) and im_cliptail.hip (the clip-tail scatter of -V), which must agree on
// which records clip to the last bit: both call clip_decide and clip_refend.  Every includer gets its own copy (unnamed namespace),
// as with im_rg.hpp.

#pragma once

#include "im_device.hpp"
#include "im_rg.hpp"

namespace im {
namespace {

constexpr int kSpanHead = 4;        // CIGAR words a lane keeps in registers; the rest come from memory

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

// The clip decision (include/indelminer_amd.h, "Clipped reads"): which ends of an eligible record are soft clips of at least
// min_clip bases.  n: the record's operations (0: not a record), kf / kl: its first / last operation that is not H.
struct ClipEnds {
    bool left, right;
    uint32_t n, kf, kl;
    uint32_t len_l, len_r;          // the clipped bases at either end (of a side that clips)
};

// a CIGAR word of a record whose cig[] holds the two words at either end (clip_decide has loaded them)
__device__ __forceinline__ uint32_t clip_word(const SpanRec& r, uint32_t n, uint32_t k)
{
    return k == 0u ? r.cig[0] : k == n - 1u ? r.cig[3] : k == 1u ? r.cig[1] : k == n - 2u ? r.cig[2] : ld_u32(r.p + r.o_cigar + 4u * k);
}

__device__ __forceinline__ ClipEnds clip_decide(SpanRec& r, int32_t n_contigs, int32_t min_clip, int32_t min_mapq)
{
    ClipEnds e; e.left = e.right = false; e.kf = e.kl = 0; e.len_l = e.len_r = 0;
    const uint32_t n = r.ok ? r.n_cigar : 0u;
    e.n = n;
    // the two words at either end, where the record has them: H may stand outside S (cig[0], cig[1]: first; cig[2], cig[3]: last)
    if (n >= 1u) { r.cig[0] = ld_u32(r.p + r.o_cigar); r.cig[3] = ld_u32(r.p + r.o_cigar + 4u * (n - 1u)); }
    if (n >= 2u) { r.cig[1] = ld_u32(r.p + r.o_cigar + 4u); r.cig[2] = ld_u32(r.p + r.o_cigar + 4u * (n - 2u)); }
    const bool eligible = n >= 1u && r.tid >= 0 && r.tid < n_contigs && !(r.flag & (0x4u | 0x100u | 0x200u | 0x400u)) && (int32_t)r.mapq >= min_mapq;
    if (eligible) {
        // first and last operation that is not H (more than one H at an end: the further words come from memory)
        uint32_t kf = 0, kl = n - 1u;
        while (kf < n && (clip_word(r, n, kf) & 15u) == 5u) kf++;
        while (kl > kf && (clip_word(r, n, kl) & 15u) == 5u) kl--;
        e.kf = kf; e.kl = kl;
        if (kf < kl) {                                              // one operation alone cannot both clip and consume reference
            const uint32_t wf = clip_word(r, n, kf), wl = clip_word(r, n, kl);
            e.left = (wf & 15u) == 4u && (int64_t)(wf >> 4) >= min_clip;
            e.right = (wl & 15u) == 4u && (int64_t)(wl >> 4) >= min_clip;
            e.len_l = wf >> 4; e.len_r = wl >> 4;
        }
    }
    return e;
}

// of a record that clips: whether its CIGAR consumes reference, and refend where the right end clips (the whole CIGAR; a left clip
// alone stops at the first operation that consumes reference and leaves *refend at pos)
__device__ __forceinline__ bool clip_refend(const SpanRec& r, const ClipEnds& e, int64_t* refend)
{
    int64_t x = r.pos;
    bool consumes = false;
    for (uint32_t k = e.kf; k <= e.kl; k++) {
        const uint32_t cw = clip_word(r, e.n, k), op = cw & 15u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) {
            consumes = true;
            if (!e.right) break;
            x += cw >> 4;
        }
    }
    *refend = x;
    return consumes;
}

}  // namespace
}  // namespace im
