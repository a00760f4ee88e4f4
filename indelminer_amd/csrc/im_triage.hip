// im_triage.hip -- fetch_func's per-record decisions for a whole chunk of BAM records on gfx950.
//
// Replaces, for every delivered record at once (src/indelminer.c:339-515):
//   the flag / pairing filters                                   348-366
//   the read-group -> range[] lookup (must_find_hashtable)       369-376
//   the three candidate cases and their mapping-quality gates    384-515
//   new_unaligned_readaln's 4-bit -> ASCII decode + revcomp      src/readaln.c:242-267, src/sequences.c:204-220
//   check_variants (CIGAR-derived evidence)                      285-337
//   the read filter and match segments of the DP= pileup         src/shared.c:160-176, bam_pileup.c:171-172
// Discordant pairs (516-615) need the host's pair table; they are only labelled here.
//
// Shape.  HBM streaming: every byte of a record is read once (core, CIGAR, aux by the record's
// own lane; the packed bases of the ~4 % candidates by the whole wave), nothing is staged.
// Four launches per chunk on the caller's stream (capturable: no memset, no allocation, no synchronisation):
//   classify   one lane per record, 64-record (one-wave) workgroups: class + read-group range per record,
//              pileup segments scattered into the genome-wide difference array, and the workgroup's
//              candidate / byte / counted / error totals as ONE plain store -- then the wave ends
//   scan       one workgroup of 256 lanes, a lane per group of 32 classify workgroups: exclusive scan of those totals on top of the running
//              candidate / byte counters (candidates are appended in RECORD ORDER -- arrival
//              order decides tie order inside clusters); one base entry per emit
//              workgroup, the running counters, the chunk's first candidate
//   emit       one lane per record: candidate index = its workgroup's base entry + position in the
//              workgroup; the owner lane writes the per-read scalars and the CIGAR-derived evidence slots
//   decode     32 lanes per candidate: the packed bases to ASCII, four bases per lane and pass
// What one launch leaves for the next is visible at the kernel boundary on the stream; no kernel
// here waits for another workgroup or reads what another workgroup of its own launch wrote.
// Algorithmic bytes: the record bytes in + (4-byte padded read + 24 B of scalars + 48 B of
// slots) per candidate out + 1 B class per record.

#include "im_device.hpp"
#include "im_rg.hpp"
#include "im_wave.hpp"

// Diagnostic build only (-DIM_STAMPS, `python indelminer_amd/build.py --stamps`): where a classify wave's life goes.  Six readings
// of the shader clock per wave -- entry, core arrived, CIGAR / aux / sweep arrived, classification done, window written out,
// publication done -- one 64-byte record per workgroup (at blockIdx.x, launches write over each other), read back through
// im_debug_tri_stamps_read by profiles/triage_stamps.py.  The product library is built without it and contains no stamp.
#ifdef IM_STAMPS
constexpr int kTriStampCap = 32768;
__device__ unsigned long long im_tri_stamp_rec[kTriStampCap][8];
#define IM_TRI_STAMP_DECL unsigned long long tri_t_[6]; tri_t_[0] = __builtin_amdgcn_s_memtime(); \
                          tri_t_[1] = tri_t_[2] = tri_t_[3] = tri_t_[4] = tri_t_[5] = tri_t_[0];
// v: a value the phase ends with -- the clock is read once it is in a register
#define IM_TRI_STAMP(k, v) do { asm volatile("" :: "v"(v)); tri_t_[k] = __builtin_amdgcn_s_memtime(); } while (0)
#define IM_TRI_STAMP_OUT(lane) do { if ((lane) < 6) { const int l_ = (lane); \
        im_tri_stamp_rec[blockIdx.x % kTriStampCap][l_] = l_ == 0 ? tri_t_[0] : l_ == 1 ? tri_t_[1] : l_ == 2 ? tri_t_[2] : l_ == 3 ? tri_t_[3] : l_ == 4 ? tri_t_[4] : tri_t_[5]; } } while (0)
#else
#define IM_TRI_STAMP_DECL
#define IM_TRI_STAMP(k, v)
#define IM_TRI_STAMP_OUT(lane)
#endif

namespace im {
namespace {

constexpr int kTriBlock = 256;          // records of an emit workgroup
constexpr int kTriGroup = 32;           // classify workgroups of a group: 256 bytes of blk[], what one lane of the scan takes a pass

__device__ __forceinline__ uint32_t ld_u16(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }

// RecView, the aux window, find_rg_mq and the read-group table: im_rg.hpp

// CIGAR word k: the first four travel in registers (one round trip with the aux window), the rest come from memory
__device__ __forceinline__ uint32_t cigar_word(const RecView& r, uint32_t k)
{
    return k == 0u ? r.cig[0] : k == 1u ? r.cig[1] : k == 2u ? r.cig[2] : k == 3u ? r.cig[3] : ld_u32(r.p + r.o_cigar + 4u * k);
}

// bam_aux2i (bam_aux.c:163-174)
__device__ __forceinline__ int32_t aux_int(const RecView& r, const AuxWin& w, uint32_t o)
{
    const uint32_t type = rec_byte(r, w, o);
    if (o + 1u >= r.len) return 0;
    const uint32_t b0 = rec_byte(r, w, o + 1);
    switch (type) {
    case 'c': return (int32_t)(int8_t)b0;
    case 'C': return (int32_t)b0;
    case 's': return (o + 3u <= r.len) ? (int32_t)(int16_t)(b0 | (rec_byte(r, w, o + 2) << 8)) : 0;
    case 'S': return (o + 3u <= r.len) ? (int32_t)(b0 | (rec_byte(r, w, o + 2) << 8)) : 0;
    case 'i': case 'I':
        return (o + 5u <= r.len) ? (int32_t)(b0 | (rec_byte(r, w, o + 2) << 8) | (rec_byte(r, w, o + 3) << 16) | (rec_byte(r, w, o + 4) << 24)) : 0;
    default: return 0;
    }
}


// new_readaln (src/readaln.c:186-240) runs for aligned proper pairs whose mate is aligned (src/indelminer.c:425), after
// the filters of 348-366: whether this record gets that far, from the core alone
__device__ __forceinline__ bool reaches_new_readaln(const RecView& r)
{
    const uint32_t f = r.flag;
    return r.ok && !(f & (0x100u | 0x200u | 0x400u | 0x800u)) && (f & 0x1u) && (f & 0x2u) && !(f & (0x4u | 0x8u)) && r.tid == r.mtid;
}

// Of eight packed bases (one dword): bit 4 p set where nibble p holds a code bit2char takes.  A popcount per nibble (the
// codes of A C G T have one bit, N has four), then "count is 1 or 4" on its three bits.
__device__ __forceinline__ uint32_t good_codes(uint32_t x)
{
    const uint32_t c = x - ((x >> 1) & 0x77777777u) - ((x >> 2) & 0x33333333u) - ((x >> 3) & 0x11111111u);
    return (c >> 2) | (c & ~(c >> 1));
}

// index (0..31) of the first refused code in 16 bytes of packed bases; only called when there is one
__device__ __forceinline__ uint32_t first_refused(const uint4& x)
{
    const uint32_t w[4] = { x.x, x.y, x.z, x.w };
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t bad = ~good_codes(w[k]) & 0x11111111u;                  // base 2 b in the high nibble of byte b
        if (bad) return 8u * k + ((uint32_t)__builtin_ctz(((bad & 0x0F0F0F0Fu) << 4) | ((bad >> 4) & 0x0F0F0F0Fu)) >> 2);
    }
    return 32u;
}

__device__ __forceinline__ bool all_good(const uint4& x)
{
    return ((good_codes(x.x) & good_codes(x.y) & good_codes(x.z) & good_codes(x.w)) & 0x11111111u) == 0x11111111u;
}

// The first base bit2char would refuse in each of a wave's 64 records, swept by the wave together: four lanes per record
// (eight when a read of the wave is longer than 128 bases) read its packed bases as consecutive 16-byte pieces.  A lane
// sweeping its own record alone makes every load a 64-line gather (measured +30 % on the whole kernel); here a load
// instruction touches 16 records.  The launch is one occupancy round -- what a wave waits for in sequence is the kernel's
// duration -- so the sweep covers l_seq bases, known from the record's core: its loads go out with the loads of the
// CIGAR and the aux window (issue), and are looked at when those have arrived (finish).  What the CIGAR makes of it
// (fewer bases, or more: new_readaln reads on behind l_seq) is settled in classify.
struct BaseSweep {
    uint4 x[8];
    uint32_t lm[8];
    int shift;      // log2 of the lanes per record: 2 or 3, the same for the whole wave
};

__device__ __forceinline__ void sweep_issue(BaseSweep& S, const uint8_t* raw, uint32_t so, uint32_t lim, int lane)
{
    S.shift = __ballot(lim > 128u) != 0ull ? 3 : 2;
    const uint32_t sub = (uint32_t)lane & ((1u << S.shift) - 1u);
    const int grp = lane >> S.shift, per_pass = 64 >> S.shift;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        S.lm[j] = 0u; S.x[j] = make_uint4(0x11111111u, 0x11111111u, 0x11111111u, 0x11111111u);
        if (j < (1 << S.shift)) {
            const int src = per_pass * j + grp;
            S.lm[j] = (uint32_t)__shfl((int)lim, src);
            const uint32_t so_j = (uint32_t)__shfl((int)so, src);
            // a lane with nothing to read takes the buffer's first bytes: the loads stay unconditional and go out together
            __builtin_memcpy(&S.x[j], raw + (32u * sub < S.lm[j] ? so_j + 16u * sub : 0u), 16);
        }
    }
}

// s_fb: the wave's 64 entries, ~0 coming in
__device__ __forceinline__ void sweep_finish(const BaseSweep& S, const uint8_t* raw, uint32_t so, uint32_t lim, uint32_t* s_fb, int lane)
{
    const uint32_t lanes = 1u << S.shift, sub = (uint32_t)lane & (lanes - 1u);
    const int grp = lane >> S.shift, per_pass = 64 >> S.shift;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j < (1 << S.shift) && 32u * sub < S.lm[j] && !all_good(S.x[j])) {
            const uint32_t idx = 32u * sub + first_refused(S.x[j]);
            if (idx < S.lm[j]) atomicMin(&s_fb[per_pass * j + grp], idx);
        }
    }
    if (__ballot(lim > 256u) != 0ull) {                                         // reads longer than 256 bases: the rest, piece by piece
        for (int j = 0; j < 8; j++) {
            const int src = per_pass * j + grp;
            const uint32_t lm = (uint32_t)__shfl((int)lim, src), so_j = (uint32_t)__shfl((int)so, src);
            for (uint32_t first = 256u + 32u * sub; first < lm; first += 256u) {
                uint4 x; __builtin_memcpy(&x, raw + so_j + (first >> 1), 16);
                if (!all_good(x)) { const uint32_t idx = first + first_refused(x); if (idx < lm) atomicMin(&s_fb[src], idx); }
            }
        }
    }
}

// CIGAR ops as bits of 1 << op: what new_readseg_bam refuses (N H P and op > 8), what carries read bases (M I S = X), what the
// pileup counts (M = X) and what moves along the reference (M D N = X)
constexpr uint32_t kOpsRefused = 0xFE68u, kOpsQuery = 0x193u, kOpsMatch = 0x181u, kOpsRef = 0x18Du;

// A 32-bit running sum that stops at 2^32 - 1.  A CIGAR has up to 65 535 ops of up to 2^28 - 1 each, so sums of lengths reach
// 2^44; every use below compares the sum with a value below 2^32 - 1, and for that the stopped sum answers as the 64-bit one does.
__device__ __forceinline__ uint32_t add_sat(uint32_t a, uint32_t b) { const uint32_t s = a + b; return s < a ? 0xFFFFFFFFu : s; }

// What the ONE walk over a record's CIGAR leaves for the rule cascade (the pileup's events go out during the walk)
struct CigarFacts {
    uint32_t seen;      // 1 << op of every op, or-ed
    uint32_t qtot;      // read bases of all ops: what new_readaln decodes, before the record's end cuts it (add_sat)
    uint32_t q0;        // read bases in front of the first refused op (add_sat)
    uint32_t nclip;     // soft clips
    bool three;         // a soft clip at the read's 3' end: the last op of a forward read, the first of a reverse one
};
struct TriageArgs {
    im_dev_records recs;
    im_dev_cands out;
    im_triage_params tp;
    RefDev ref;
    RgTable rg;
    int32_t* depth_diff;    // genome-wide difference array (index = ascii offset of the position) or null
    uint32_t* info;         // [n] class | revcomp << 8
    int32_t* rmax;          // [n]
    uint2* blk;             // [classify workgroups, padded to whole groups of kTriGroup] one packed word per workgroup: x = candidates | counted << 9 | errors << 18, y = padded read bytes
    uint2* wg_base;         // [emit workgroups] candidates / bytes in front of an emit workgroup (running counters included), written by the scan
    uint32_t* seq_at;       // [cap_cand] byte offset of a candidate's packed bases in recs.raw, | 1 << 31 = reverse complement
    int32_t* chunk_base;    // [1] candidates before this chunk (written by the scan)
};

__device__ __forceinline__ uint32_t padded4(int32_t l) { return ((uint32_t)l + 3u) & ~3u; }

// The classify kernel runs in ONE-WAVE workgroups that hold at most kClsLdsBudget bytes of LDS: realign_kernel<6, true> is one wave
// and 6 352 B (allocated as 6 400) per workgroup, and while a realign launch of another stream still has workgroups pending, the
// holes its retiring waves leave on a CU are that size -- a workgroup that needs more starts only where realign has drained
// (profiles/README.md, "classify beside realign").  One wave also means no barrier, and the per-wave totals stay in registers.
constexpr int kClsBlock = 64;
constexpr int kClsLdsBudget = 6400;
constexpr int kDepthWin = 1024;     // positions of the depth difference array a workgroup gathers in LDS before it touches memory:
                                    // 16 per record.  Events outside it go to memory directly, so results do not depend on it.
constexpr int kClsRgLds = 448;      // an insert-length table up to this size (a handful of read groups) is copied to LDS
static_assert(kTriBlock % kClsBlock == 0 && kTriGroup % (kTriBlock / kClsBlock) == 0, "an emit workgroup's classify blocks lie in one group");
static_assert(kClsBlock < 512, "a workgroup's candidate, counted and error counts take nine bits each of its packed word");
static_assert(kClsBlock * kAuxWin + kClsBlock * 4 + kDepthWin * 4 + kClsRgLds <= kClsLdsBudget, "classify must fit the hole a realign wave leaves");

// LDS written by one lane and read by another of the same wave: the wave's LDS operations complete in order, so only the
// compiler has to keep them in order.  Wavefront scope: no barrier, no cache operation.
__device__ __forceinline__ void wave_lds_order() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

__global__ __launch_bounds__(kClsBlock, 6) void triage_classify_kernel(TriageArgs A)
{
    __shared__ uint32_t s_aux[kClsBlock][kAuxWin / 4];
    __shared__ uint32_t s_rg[kClsRgLds / 4];
    // The pileup's +1 / -1 of this workgroup's records, gathered here first: a coordinate-sorted BAM puts the 64 records of
    // a workgroup within a few hundred positions of each other, so their ~128 scattered device atomics become LDS adds and
    // a few whole-line atomic instructions (measured: the scatter was 45 us of a 300 000-record launch, as much as the
    // rest of the kernel).  Events outside the window or on another contig go to memory directly.
    __shared__ int32_t s_dd[kDepthWin];
    __shared__ uint32_t s_fb[kClsBlock];
    const int lane = threadIdx.x;
    IM_TRI_STAMP_DECL
    const int64_t i = (int64_t)blockIdx.x * kClsBlock + lane;
    if (A.depth_diff) {
        int4* z = reinterpret_cast<int4*>(s_dd);
#pragma unroll
        for (int k = 0; k < kDepthWin / 4 / kClsBlock; k++) z[lane + k * kClsBlock] = make_int4(0, 0, 0, 0);
    }

    // the record: offsets, core, then CIGAR head + aux window + the wave's sweep over the packed bases in one round trip
    RecView r; r.ok = false; r.l_seq = 0; r.flag = 0; r.n_cigar = 0; r.tid = -1; r.pos = 0; r.o_cigar = 0; r.o_seq = 0; r.p = A.recs.raw; r.len = 0; r.o_aux = 0;
    r.mtid = -1; r.isize = 0; r.mapq = 0;
    s_fb[lane] = 0xFFFFFFFFu;
    // the insert-length table: LDS copy when it is small (its loads go out with the record offsets')
    const bool rg_lds = A.rg.bytes <= kClsRgLds;
    if (rg_lds) for (int k = lane; 4 * k < A.rg.bytes; k += kClsBlock) s_rg[k] = reinterpret_cast<const uint32_t*>(A.rg.blob)[k];
    const bool valid = i < A.recs.n;
    if (valid) r = view_record(A.recs.raw, A.recs.rec_off[i], A.recs.rec_off[i + 1]);
    IM_TRI_STAMP(1, r.flag);
    const bool pp = reaches_new_readaln(r);                                     // r.ok: the packed bases lie inside the record
    const uint32_t sw_lim = pp ? (uint32_t)r.l_seq : 0u;
    const uint32_t sw_so = sw_lim ? (uint32_t)(r.p - A.recs.raw) + r.o_seq : 0u;
    BaseSweep S;
    sweep_issue(S, A.recs.raw, sw_so, sw_lim, lane);
    {
        // The CIGAR head and the aux window: ten loads that go out together and are waited for once.  They are unconditional: a
        // lane without a record takes the buffer's first bytes (the chunk holds >= 64), a record with a short aux area reads on
        // behind it -- at most 24 bytes behind the record, inside the chunk buffer's >= 64 spare bytes -- and what lands in the
        // window for bytes the aux area does not have is never looked at: every reader checks its offset against r.len first.
        const uint8_t* pc = r.ok ? r.p + r.o_cigar : A.recs.raw;
        const uint8_t* pa = r.ok ? r.p + r.o_aux : A.recs.raw;
        uint32_t av[kAuxWin / 4];
#pragma unroll
        for (int k = 0; k < 4; k++) r.cig[k] = ld_u32(pc + 4u * k);
#pragma unroll
        for (int k = 0; k < kAuxWin / 4; k++) av[k] = ld_u32(pa + 4u * k);
#pragma unroll
        for (int k = 0; k < kAuxWin / 4; k++) s_aux[lane][k] = av[k];
    }
    wave_lds_order();                                                           // s_fb's ~0 before the sweep's minima
    sweep_finish(S, A.recs.raw, sw_so, sw_lim, s_fb, lane);
    // the depth window starts at the first pileup-eligible record of the workgroup (records are sorted inside a contig)
    const bool piles = A.depth_diff && r.ok && r.tid >= 0 && r.tid < A.ref.n_contigs && !(r.flag & (0x4u | 0x100u | 0x200u | 0x400u));
    int32_t dd_pos = 0, dd_tid = -1;
    int64_t pl_base = 0;            // the lane's contig in the difference array
    uint32_t pl_end = 0;            // and its length, as a biased position (below)
    if (A.depth_diff) {
        const uint64_t mp = __ballot(piles);
        const int first = mp ? (int)__builtin_ctzll(mp) : 0;
        const int fp = __shfl(r.pos, first), ft = __shfl(r.tid, first);
        dd_pos = fp < 0 ? 0 : fp; dd_tid = mp ? ft : -1;
        if (mp) {
            // a lane that does not pile up asks for the window's contig: the loads stay unconditional
            const int32_t t = piles ? r.tid : dd_tid;
            pl_base = A.ref.asc_off[t];
            pl_end = (uint32_t)A.ref.len[t] ^ 0x80000000u;
        }
    }
    wave_lds_order();                                                           // the table, the sweep's minima and the zeroed window are in
    IM_TRI_STAMP(2, r.cig[3]);
    const RgView T = rg_view(rg_lds ? reinterpret_cast<const uint8_t*>(s_rg) : A.rg.blob, A.rg.n);

    // ---- the rules' inputs (src/indelminer.c:348-366): computed by every lane, nothing branches on them
    const uint32_t flag = r.flag;
    const bool aligned = !(flag & 0x4u), mate_aligned = !(flag & 0x8u), both = aligned && mate_aligned;
    const bool proper = (flag & 0x2u) != 0, is_rc = (flag & 0x10u) != 0, mate_rc = (flag & 0x20u) != 0;
    // past the flag / pairing filters: the record counts, and its tags are looked at
    const bool counted = r.ok && !(flag & (0x100u | 0x200u | 0x400u | 0x800u)) && (flag & 0x1u) && !(both && r.tid != r.mtid);

    // ---- the ONE walk over the CIGAR: a loop of the wave's, to the longest CIGAR among the lanes that need theirs (proper pairs
    // for new_readaln's census, pileup-eligible records for their match segments).  Per op a lane takes
    //   seen, nclip, three   the census of src/indelminer.c:441-460
    //   q / q0               read bases so far / in front of the first op new_readseg_bam refuses
    //   u                    the reference position, and from it the pileup's +1 / -1 of an M = X run
    // Value ranges.  q: add_sat (above).  u is the position x = pos + (lengths so far) as x + 2^31 in a uint32 with add_sat: pos is
    // an int32, so the bias makes it non-negative, and a sum stopped at 2^32 - 1 stands for "x >= 2^31 - 1", which is at or
    // behind every contig's end (len is an int32): max(x, 0) and min(x + len, clen) of the 64-bit form become max / min against
    // the biased 0 and the biased clen, with the same outcome of a < b and the same a and b wherever a < b.
    CigarFacts cf; cf.seen = 0u; cf.qtot = 0u; cf.q0 = 0u; cf.nclip = 0u; cf.three = false;
    {
        const uint32_t nc = (pp || piles) ? r.n_cigar : 0u;
        const uint32_t nmax = (uint32_t)wave_max((int)nc);                      // n_cigar < 2^16
        const uint32_t three_at = is_rc ? 0u : r.n_cigar - 1u;
        const bool here = r.tid == dd_tid;
        uint32_t u = (uint32_t)r.pos ^ 0x80000000u;
        auto op_step = [&](uint32_t k, uint32_t cw) {
            const uint32_t bit = k < nc ? 1u << (cw & 15u) : 0u, len = cw >> 4;
            if ((bit & kOpsRefused) && !(cf.seen & kOpsRefused)) cf.q0 = cf.qtot;
            cf.seen |= bit;
            cf.qtot = add_sat(cf.qtot, (bit & kOpsQuery) ? len : 0u);
            cf.nclip += (bit >> 4) & 1u;
            cf.three = cf.three || ((bit & 16u) && k == three_at);
            const uint32_t ue = add_sat(u, (bit & kOpsRef) ? len : 0u);
            // what samtools' pileup counts (bam_pileup.c:171-172, 238-265): M/=/X of records that are mapped, primary, not
            // QC-failed, not duplicates -- whatever class the record gets
            const uint32_t au = u > 0x80000000u ? u : 0x80000000u, bu = ue < pl_end ? ue : pl_end;
            if (piles && (bit & kOpsMatch) && au < bu) {
                // 0 <= a < b <= clen < 2^31, dd_pos >= 0: the differences fit an int32, and as uint32 one compare is "0 <= . < window"
                const int32_t a = (int32_t)(au ^ 0x80000000u), b = (int32_t)(bu ^ 0x80000000u);
                const uint32_t ra = (uint32_t)(a - dd_pos), rb = (uint32_t)(b - dd_pos);
                // the array index keeps 64 bits in its last addition
                if (here && ra < (uint32_t)kDepthWin) atomicAdd(&s_dd[ra], 1); else atomicAdd(&A.depth_diff[pl_base + a], 1);
                if (here && rb < (uint32_t)kDepthWin) atomicAdd(&s_dd[rb], -1); else atomicAdd(&A.depth_diff[pl_base + b], -1);
            }
            u = ue;
        };
        // the first four words travel in registers (one round trip with the aux window) ...
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) if (k < nmax) op_step(k, r.cig[k]);
        // ... the rest come from memory, for the lanes that have them
        for (uint32_t k = 4u; k < nmax; k++) {
            uint32_t cw = 0u;
            if (k < nc) cw = ld_u32(r.p + r.o_cigar + 4u * k);
            op_step(k, cw);
        }
    }

    // ---- the tags (369-376, and the MQ of 386-424 / 461): one walk of the wave's for RG and MQ
    AuxWin w; w.lds = s_aux[lane]; w.o0 = r.o_aux;
    uint32_t o_rg, o_mq;
    find_rg_mq(r, w, o_rg, o_mq, counted);
    // the read group's range.  No RG tag: "generic", looked up once per workgroup.  A tag: behind a test of the wave's
    const bool defer = A.tp.defer_ranges != 0;      // the table is still being estimated: only what does not need it is checked
    const bool has_rg = counted && o_rg != 0u;
    const bool generic = counted && !has_rg && !defer;
    bool rg_err = generic && A.rg.generic_ok == 0;
    int32_t rmax = (generic && A.rg.generic_ok != 0) ? A.rg.generic_range : 0;
    if (__ballot(has_rg) != 0ull) {
        if (has_rg) {
            if (defer) { const uint32_t type = rec_byte(r, w, o_rg); rg_err = !(type == 'Z' || type == 'H'); }   // a type bam_aux2Z refuses
            else { int32_t rm = 0; if (rg_tag_range(r, w, o_rg, T, rm)) rmax = rm; else rg_err = true; }
        }
    }
    const bool live = counted && !rg_err;
    const bool um = live && !aligned && mate_aligned;                           // 386-424
    const bool ppl = live && both && proper;                                    // 425-515
    const bool pe = live && both && !proper;                                    // 516-521

    // ---- proper pairs.  new_readaln (src/readaln.c:186-240) builds the segment list of EVERY proper pair first, op by op: N / H / P
    // and unknown ops are fatal (163-182), and so is a base code other than A C G T N in an op that carries read bases (bit2char,
    // 4-16) -- whichever comes first along the CIGAR.  s_fb holds the first bad base among the l_seq bases of the read (the wave's
    // cooperative sweep); only what lies inside the CIGAR's reach counts -- the query bases of all ops, taken where the CIGAR says,
    // also past l_seq, but not past the record -- and a CIGAR that reaches past l_seq has the bytes behind the packed bases looked
    // at here.  A bad op at read offset q0 loses to a bad base in front of it.
    // r.len < 2^31 (chunk offsets fit 31 bits: seq_at), so twice the bytes behind o_seq fit 32 bits; qtot stopped at 2^32 - 1 is
    // above that, and the minimum is the 64-bit one
    const uint32_t avail = 2u * (r.len - r.o_seq);
    const uint32_t lim = cf.qtot < avail ? cf.qtot : avail;
    uint32_t fb = s_fb[lane];
    fb = fb >= lim ? 0xFFFFFFFFu : fb;
    const bool behind = ppl && fb == 0xFFFFFFFFu && lim > (uint32_t)r.l_seq;
    if (__ballot(behind) != 0ull) {
        if (behind) {
            for (uint32_t j = (uint32_t)r.l_seq; j < lim; j++) {
                const uint32_t code = (r.p[r.o_seq + (j >> 1)] >> ((~j & 1u) << 2)) & 15u;
                if (!(code == 1u || code == 2u || code == 4u || code == 8u || code == 15u)) { fb = j; break; }
            }
        }
    }
    // fb < lim < 2^32 - 1 or fb = ~0: against q0 stopped at 2^32 - 1 "a bad base in front of the op" is fb < q0 as it is in 64 bits,
    // and "no bad base" (~0) is in front of nothing, also where the op lies 2^32 or more read bases in: IM_REC_ERR_CIGAR, as the
    // reference has it
    const uint32_t pp_err = (cf.seen & kOpsRefused) ? (fb < cf.q0 ? IM_REC_ERR_BASE : IM_REC_ERR_CIGAR) : fb != 0xFFFFFFFFu ? IM_REC_ERR_BASE : 0u;
    // 441-460: an indel, or a clip other than the one clip at the 3' end
    const bool variant = (cf.seen & 6u) != 0u || cf.nclip > 1u || (cf.nclip == 1u && !cf.three);

    // ---- the mate's mapping quality: the MQ tag where there is one, for the records whose class hangs on it.  An MQ:C inside the
    // window (what aligners write) is one LDS byte; any other type, or a tag the window has left, behind a test of the wave's
    const bool need_mq = o_mq != 0u && (um || (ppl && pp_err == 0u && variant));
    const bool mq_in = need_mq && aux_covers(w, o_mq, 2u);                      // o_mq + 1 < r.len: a field has at least four bytes
    const uint32_t mq_type = win_byte(w, o_mq, mq_in), mq_byte = win_byte(w, o_mq + 1u, mq_in);
    const bool mq_fast = mq_in && mq_type == 'C';
    int32_t mmq = mq_fast ? (int32_t)mq_byte : (int32_t)r.mapq;
    bool mq_err = false;
    const bool mq_slow = need_mq && !mq_fast;
    if (__ballot(mq_slow) != 0ull) {
        if (mq_slow) {
            aux_cover(r, w, o_mq, 5u);
            const uint32_t t = rec_byte(r, w, o_mq);
            // only the unmapped-read case checks the type (399-403); a proper pair takes bam_aux2i's 0
            mq_err = um && !(t == 'I' || t == 'i' || t == 'C' || t == 'c' || t == 'S' || t == 's');
            mmq = aux_int(r, w, o_mq);
        }
    }
    const bool mq_pass = mmq >= A.tp.qthreshold;

    // ---- the class, in the reference's order of precedence
    // 516-521: abs(isize) as an int against range_max, as a uint against maxpedelsize.  |isize| <= 2^31 is exact in a uint32; a
    // negative range_max is below it, and a non-negative one compares as a uint32 as it does in 64 bits
    const uint32_t a32 = r.isize < 0 ? 0u - (uint32_t)r.isize : (uint32_t)r.isize;
    const bool pe_hit = (rmax < 0 || a32 > (uint32_t)rmax) && a32 < A.tp.maxpedelsize && is_rc != mate_rc;
    uint32_t cls = !valid ? IM_REC_SKIP : !r.ok ? IM_REC_ERR_LIMIT : !counted ? IM_REC_SKIP : rg_err ? IM_REC_ERR_RG : IM_REC_COUNTED;
    bool revcomp = false;
    if (um) { cls = mq_err ? IM_REC_ERR_MQ : mq_pass ? IM_REC_CAND_UNMAPPED : IM_REC_COUNTED; revcomp = !mq_err && mq_pass && !mate_rc; }
    if (ppl) {
        const bool hit = pp_err == 0u && variant && mq_pass;
        cls = pp_err != 0u ? pp_err : hit ? IM_REC_CAND_PROPER : IM_REC_COUNTED;
        revcomp = hit && is_rc == mate_rc;
    }
    if (pe && pe_hit) cls = IM_REC_PE;
    const bool cand = cls == IM_REC_CAND_UNMAPPED || cls == IM_REC_CAND_PROPER;
    const uint32_t bytes = cand ? padded4(r.l_seq) : 0u;
    if (valid) {
        A.info[i] = cls | (revcomp ? 0x100u : 0u);
        A.rmax[i] = rmax;
        if (A.out.rec_class) A.out.rec_class[i] = (uint8_t)cls;
    }
    IM_TRI_STAMP(3, cls);
    // workgroup totals
    const uint64_t mc = __ballot(cand);
    uint32_t wb = bytes;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wb += (uint32_t)__shfl_xor((int)wb, o);
    const uint64_t mk = __ballot(cls != IM_REC_SKIP), me = __ballot(cls >= IM_REC_ERR_RG);
    wave_lds_order();                                                           // every lane's window adds before the window goes out
    if (A.depth_diff && dd_tid >= 0) {
        // the gathered window out: consecutive lanes hold consecutive positions, only non-zero entries touch memory
        int32_t* dst = A.depth_diff + A.ref.asc_off[dd_tid] + dd_pos;
        const int64_t room = (int64_t)A.ref.len[dd_tid] + 1 - dd_pos;          // the contig's run has len + 1 entries
#pragma unroll 4
        for (int k = 0; k < kDepthWin / kClsBlock; k++) {
            const int idx = lane + k * kClsBlock;
            const int32_t v = s_dd[idx];
            if (v != 0 && idx < room) atomicAdd(&dst[idx], v);
        }
    }
    IM_TRI_STAMP(4, wb);
    // Publication: the workgroup's totals in one packed word, one plain store by lane 0, and the wave ends -- it holds its registers
    // and its LDS for no round trip after its last store.  The scan launch behind this one on the stream reads the words; the kernel
    // boundary makes them visible.  (Until the scan had a launch of its own again, every wave counted itself into its group with two
    // dependent returning atomics, and the last wave of the launch scanned: profiles/README.md, "the scan out of classify's waves".)
    // x: candidates, counted records and error records (each <= 64; 9 bits each); y: padded read bytes
    if (lane == 0) A.blk[blockIdx.x] = make_uint2((uint32_t)__popcll(mc) | ((uint32_t)__popcll(mk) << 9) | ((uint32_t)__popcll(me) << 18), wb);
    IM_TRI_STAMP(5, wb);
    IM_TRI_STAMP_OUT(lane);
}

// The scan: ONE workgroup of kScanLanes lanes, two levels.  A lane takes one GROUP of kTriGroup classify workgroups a pass: the
// kAhead emit workgroups they make, kScanPerLane words each, 256 consecutive bytes of blk[] as sixteen loads that are in flight
// together.  It adds them up per emit workgroup, the groups' totals are scanned across the workgroup (DPP steps inside a wave, the
// waves' totals through LDS, one barrier), and the lane walks its emit workgroups again, writing each one's base where
// triage_emit_kernel takes it with one load.  A pass covers kScanLanes groups = 8 192 classify workgroups = 524 288 records, so the
// launches of the product's chunks are one pass.  A longer launch takes pass after pass; fetching the next pass's words before the
// current pass is scanned was built and measured, and did not pay (143 registers against 94, and no faster on a launch of four
// passes: profiles/README.md).  At most 256 lanes: a wider workgroup starts only where a CU has room for all of its waves, and
// beside the other streams' one-wave workgroups that took up to 58 us (profiles/README.md).
constexpr int kScanLanes = 256;
constexpr int kScanPerLane = kTriBlock / kClsBlock;
constexpr int kAhead = 8;
static_assert(kScanPerLane == 4, "an emit workgroup's words are two 16-byte loads");
static_assert(kAhead * kScanPerLane == kTriGroup, "a lane's kAhead emit workgroups are one group");
static_assert(kTriGroup * sizeof(uint2) == 256, "blk[] is padded to 256 bytes: whole groups");
static_assert(kScanLanes % 64 == 0 && kScanLanes <= 256, "whole waves, and no wider than fits beside the other streams' workgroups");

__global__ __launch_bounds__(kScanLanes) void triage_scan_kernel(TriageArgs A)
{
    constexpr int kWaves = kScanLanes / 64;
    __shared__ uint2 s_tot[2][kWaves];              // the waves' totals of a pass; passes alternate between the two rows (one barrier a pass)
    __shared__ uint2 s_ke[kWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int32_t n_blocks = (int32_t)(((int64_t)A.recs.n + kClsBlock - 1) / kClsBlock);
    const int32_t n_emit = (n_blocks + kScanPerLane - 1) / kScanPerLane;
    const int32_t n_groups = (n_blocks + kTriGroup - 1) / kTriGroup;
    const int32_t n_passes = (n_groups + kScanLanes - 1) / kScanLanes;
    // restart: this launch opens a new batch -- the running counters count as zero whatever they hold (no memset in front)
    const bool fresh = A.tp.restart != 0;
    uint32_t carry_c = fresh ? 0u : (uint32_t)A.out.counters[0], carry_b = fresh ? 0u : (uint32_t)A.out.counters[1];
    const uint32_t chunk_first = carry_c;
    const uint4* src = reinterpret_cast<const uint4*>(A.blk);           // two workgroups' words a load
    uint4 buf[2 * kAhead];
    // blk[] is allocated in whole groups (256 bytes).  A lane behind the launch's last group loads that group again -- the loads
    // stay unconditional -- and counts none of it
    auto fetch = [&](int32_t pass) {
        const int64_t g = (int64_t)pass * kScanLanes + t;
        const uint4* p = src + (g < n_groups ? g : (int64_t)n_groups - 1) * (2 * kAhead);
#pragma unroll
        for (int i = 0; i < 2 * kAhead; i++) buf[i] = p[i];
    };
    uint32_t sum_k = 0, sum_e = 0;
    for (int32_t pass = 0; pass < n_passes; pass++) {
        fetch(pass);
        const int64_t g = (int64_t)pass * kScanLanes + t;
        // classify and emit workgroups of the launch inside this lane's group
        const int64_t left_b = (int64_t)n_blocks - g * kTriGroup, left_e = (int64_t)n_emit - g * kAhead;
        const int nb = left_b < 0 ? 0 : left_b > kTriGroup ? kTriGroup : (int)left_b, ne = left_e < 0 ? 0 : left_e > kAhead ? kAhead : (int)left_e;
        // the lane's emit workgroups: candidates and bytes of each.  Words of classify workgroups behind the launch's last one are
        // whatever an earlier, larger launch left there: they count as zero
        uint32_t oc[kAhead], ob[kAhead], own_c = 0, own_b = 0;
#pragma unroll
        for (int j = 0; j < kAhead; j++) {
            const uint4 d0 = buf[2 * j], d1 = buf[2 * j + 1];
            const uint32_t wx[4] = { d0.x, d0.z, d1.x, d1.z }, wy[4] = { d0.y, d0.w, d1.y, d1.w };
            oc[j] = 0u; ob[j] = 0u;
#pragma unroll
            for (int k = 0; k < kScanPerLane; k++) {
                const bool in = j * kScanPerLane + k < nb;
                const uint32_t x = in ? wx[k] : 0u;
                oc[j] += x & 511u; ob[j] += in ? wy[k] : 0u;
                sum_k += (x >> 9) & 511u; sum_e += (x >> 18) & 511u;
            }
            own_c += oc[j]; own_b += ob[j];
        }
        const uint32_t c = (uint32_t)wave_scan_add((int)own_c, lane), b = (uint32_t)wave_scan_add((int)own_b, lane);
        uint2* tot = s_tot[pass & 1];
        if (lane == 63) tot[wave] = make_uint2(c, b);
        __syncthreads();
        uint32_t front_c = 0, front_b = 0, all_c = 0, all_b = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            const uint2 v = tot[w];
            if (w < wave) { front_c += v.x; front_b += v.y; }
            all_c += v.x; all_b += v.y;
        }
        uint32_t at_c = carry_c + front_c + c - own_c, at_b = carry_b + front_b + b - own_b;
#pragma unroll
        for (int j = 0; j < kAhead; j++) {
            if (j < ne) A.wg_base[g * kAhead + j] = make_uint2(at_c, at_b);
            at_c += oc[j]; at_b += ob[j];
        }
        carry_c += all_c; carry_b += all_b;
    }
    sum_k = (uint32_t)wave_sum((int)sum_k); sum_e = (uint32_t)wave_sum((int)sum_e);
    if (lane == 0) s_ke[wave] = make_uint2(sum_k, sum_e);
    __syncthreads();
    if (t == 0) {
        uint32_t k = 0, e = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) { k += s_ke[w].x; e += s_ke[w].y; }
        A.chunk_base[0] = (int32_t)chunk_first;
        const int32_t k0 = fresh ? 0 : A.out.counters[2], e0 = fresh ? 0 : A.out.counters[3];
        A.out.counters[0] = (int32_t)carry_c; A.out.counters[1] = (int32_t)carry_b;
        A.out.counters[2] = k0 + (int32_t)k;                                           // records counted
        A.out.counters[3] = e0 + (int32_t)e;                                           // error records (emit / decode add theirs later)
        if (fresh) A.out.counters[4] = 0;                                              // overflows: counted by the emit kernel
    }
}

// 4-bit base code -> ASCII (bit2char, src/readaln.c:4-17); 0 = a code the reference exits on
__device__ __forceinline__ uint32_t base_ascii(uint32_t code)
{
    return code == 1u ? 'A' : code == 2u ? 'C' : code == 4u ? 'G' : code == 8u ? 'T' : code == 15u ? 'N' : 0u;
}
// complement in code space (A<->T, C<->G, N<->N: src/sequences.c:22-26) = reversal of the four bits
__device__ __forceinline__ uint32_t comp_code(uint32_t c) { return ((c & 1u) << 3) | ((c & 2u) << 1) | ((c & 4u) >> 1) | ((c & 8u) >> 3); }

// per candidate, by the lane that owns its record: place in the batch, scalars, CIGAR-derived evidence slots
__global__ __launch_bounds__(kTriBlock) void triage_emit_kernel(TriageArgs A)
{
    __shared__ uint32_t s_cnt[kTriBlock / 64], s_bytes[kTriBlock / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t i = (int64_t)blockIdx.x * kTriBlock + t;
    uint32_t info = 0;
    RecView r; r.ok = false; r.l_seq = 0; r.o_seq = 0; r.p = A.recs.raw;
    if (i < A.recs.n) {
        info = A.info[i];
        const uint32_t cls = info & 255u;
        if (cls == IM_REC_CAND_UNMAPPED || cls == IM_REC_CAND_PROPER) {
            r = view_record(A.recs.raw, A.recs.rec_off[i], A.recs.rec_off[i + 1]);
#pragma unroll
            for (int k = 0; k < 4; k++) r.cig[k] = ld_u32(r.p + r.o_cigar + 4u * k);
        }
    }
    const bool cand = r.ok;
    const uint32_t bytes = cand ? padded4(r.l_seq) : 0u;
    // position among the workgroup's candidates / bytes
    const uint64_t mc = __ballot(cand);
    const uint32_t below = (uint32_t)__popcll(mc & ((1ull << lane) - 1ull));
    uint32_t ib = bytes;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t tb = (uint32_t)__shfl_up((int)ib, o); if (lane >= o) ib += tb; }
    if (lane == 63) { s_cnt[wave] = (uint32_t)__popcll(mc); s_bytes[wave] = ib; }
    __syncthreads();
    if (!cand) return;
    uint32_t oc = 0, ob = 0;
    for (int w = 0; w < wave; w++) { oc += s_cnt[w]; ob += s_bytes[w]; }
    const uint2 base = A.wg_base[blockIdx.x];           // candidates / bytes in front of this workgroup, running counters included (the scan)
    const uint32_t ci = base.x + oc + below;
    const uint32_t bo = base.y + ob + ib - bytes;
    const im_dev_batch& B = A.out.batch;
    if (!(ci < (uint32_t)A.out.cap_cand && (uint64_t)bo + bytes + 16u <= (uint64_t)A.out.cap_bases)) {
        atomicAdd(&A.out.counters[4], 1);
        // The decode kernel walks every candidate below min(counters[0], cap_cand): one whose bases do not fit gets the
        // length 0 there, so that nothing is read or written for it (its words would hold what an earlier batch left)
        if (ci < (uint32_t)A.out.cap_cand) {
            const_cast<int64_t*>(B.base_off)[ci] = 0;
            const_cast<int32_t*>(B.read_len)[ci] = 0;
            A.seq_at[ci - (uint32_t)A.chunk_base[0]] = 0u;
        }
        return;
    }
    const_cast<int64_t*>(B.base_off)[ci] = (int64_t)bo;
    const_cast<int32_t*>(B.read_len)[ci] = r.l_seq;
    const_cast<int32_t*>(B.tid)[ci] = r.mtid;
    const_cast<int32_t*>(B.anchor)[ci] = r.mpos;
    const_cast<int32_t*>(B.range_max)[ci] = A.rmax[i];
    A.out.cand_rec[ci] = A.recs.rec_base + (int32_t)i;
    // chunk offsets fit 31 bits (chunks are far below 2 GiB); indexed by the candidate's place in THIS chunk
    A.seq_at[ci - (uint32_t)A.chunk_base[0]] = ((uint32_t)(r.p - A.recs.raw) + r.o_seq) | ((info & 0x100u) ? 0x80000000u : 0u);
    // check_variants (src/indelminer.c:285-337): one evidence per I / D op that is far enough from both ends
    int ne = 0;
    uint32_t err = 0;
    int32_t e_cls[IM_MAX_EV] = { -1, -1, -1, -1 }, e_b1[IM_MAX_EV] = { 0, 0, 0, 0 }, e_b2[IM_MAX_EV] = { 0, 0, 0, 0 };
    if ((info & 255u) == IM_REC_CAND_PROPER) {
        uint32_t tpos = 0, rpos = 0;
        for (uint32_t k = 0; k < r.n_cigar; k++) {
            const uint32_t w = cigar_word(r, k), op = w & 15u;
            if (op == 7u || op == 8u || op == 0u || op == 1u) tpos += w >> 4;
        }
        int32_t refpos = r.pos;
        bool over = false;      // more evidence than the slots hold: the kernel's own limit, behind anything the reference refuses further on
        for (uint32_t k = 0; k < r.n_cigar && !err; k++) {
            const uint32_t w = cigar_word(r, k), op = w & 15u, len = w >> 4;
            if (op == 2u || op == 1u) {
                if (rpos > A.tp.ethreshold_vcfcheck && (tpos - rpos) > A.tp.ethreshold_vcfcheck) {
                    const int32_t c = op == 2u ? IM_CLS_DELETION : IM_CLS_INSERTION, x1 = refpos, x2 = op == 2u ? refpos + (int32_t)len : refpos;
                    // static slot selection keeps the three small arrays in registers
                    if (ne == 0) { e_cls[0] = c; e_b1[0] = x1; e_b2[0] = x2; }
                    else if (ne == 1) { e_cls[1] = c; e_b1[1] = x1; e_b2[1] = x2; }
                    else if (ne == 2) { e_cls[2] = c; e_b1[2] = x1; e_b2[2] = x2; }
                    else if (ne == 3) { e_cls[3] = c; e_b1[3] = x1; e_b2[3] = x2; }
                    else over = true;
                    ne += ne < IM_MAX_EV ? 1 : 0;
                }
            } else if (op == 0u || op == 7u || op == 8u) rpos += len;
            else if (op == 4u) { if (!(k == 0u || k == r.n_cigar - 1u)) err = IM_REC_ERR_CLIP; }
            else err = IM_REC_ERR_CIGAR;
            if (op == 0u || op == 7u || op == 8u || op == 2u) refpos += (int32_t)len;
        }
        if (!err && over) err = IM_REC_ERR_LIMIT;
    }
    if (B.ev_cls) {
#pragma unroll
        for (int k = 0; k < IM_MAX_EV; k++) {
            const int64_t sl = (int64_t)ci * IM_MAX_EV + k;
            if (A.out.consumed) A.out.consumed[sl] = 0;        // a fresh candidate: no flush has consumed its evidence
            B.ev_cls[sl] = err ? -1 : e_cls[k];
            B.ev_b1[sl] = err ? 0 : e_b1[k];
            B.ev_b2[sl] = err ? 0 : e_b2[k];
        }
    }
    if (err) {
        A.info[i] = (info & ~255u) | err;                      // the decode below leaves a record that already failed alone
        if (A.out.rec_class) A.out.rec_class[i] = (uint8_t)err;
        atomicAdd(&A.out.counters[3], 1);
    }
}

// new_unaligned_readaln's decode (src/readaln.c:242-267) + reverse_complement_string (src/sequences.c:204-220) for the
// chunk's candidates, 32 lanes per read, four bases per lane and pass: candidates cluster around the indel sites, so
// the work is spread over the candidate list and not over the records (decoding inside the emit kernel, each wave its own
// candidates one after the other, was tried in round 4: a wave at an indel site holds thirty candidates, its neighbours none --
// 57 us against 6.2 + 5.6 at 300 000 records, 103 against 15 + 20 at 1.875 M)
__global__ __launch_bounds__(256) void triage_decode_kernel(TriageArgs A)
{
    const int sub = threadIdx.x >> 5, l32 = threadIdx.x & 31;
    const int32_t c0 = A.chunk_base[0];
    const int32_t c1 = min(A.out.counters[0], A.out.cap_cand);
    for (int32_t ci = c0 + (int32_t)blockIdx.x * 8 + sub; ci < c1; ci += (int32_t)gridDim.x * 8) {
        const uint32_t at = A.seq_at[ci - c0];
        const bool rc = (at & 0x80000000u) != 0;
        const uint8_t* seq = A.recs.raw + (at & 0x7FFFFFFFu);
        const int32_t L = A.out.batch.read_len[ci];
        uint8_t* dst = const_cast<uint8_t*>(A.out.batch.bases) + A.out.batch.base_off[ci];
        bool bad = false;
        for (int32_t p0 = 4 * l32; p0 < (int32_t)padded4(L); p0 += 128) {
            // the lane's (up to) four bases in ONE load: forwards they are two bytes (p0 is even), backwards they lie in the
            // three bytes from that of the last base on -- four bytes from there stay inside the record or the chunk's slack
            const int32_t n_here = min(4, L - p0);
            const int32_t qlo = rc ? L - p0 - n_here : p0;
            const uint32_t packed = rc ? ld_u32(seq + (qlo >> 1)) : ld_u16(seq + (p0 >> 1));
            const int32_t b0 = qlo >> 1;
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (j >= n_here) break;
                const int32_t q = rc ? L - 1 - p0 - j : p0 + j;
                const uint32_t byte = (packed >> (8 * ((q >> 1) - b0))) & 255u;
                uint32_t code = (q & 1) ? (byte & 15u) : (byte >> 4);
                if (rc) code = comp_code(code);
                const uint32_t ch = base_ascii(code);
                bad |= ch == 0u;
                word |= ch << (8 * j);
            }
            *reinterpret_cast<uint32_t*>(dst + p0) = word;
        }
        // a base code the reference exits on (bit2char): the candidate's record gets the error class
        const uint64_t mb = __ballot(bad);
        const uint32_t half = (uint32_t)(mb >> (32 * ((threadIdx.x >> 5) & 1)));
        if (half != 0u && l32 == 0) {
            // check_variants comes first in the reference (src/indelminer.c:470 before 484): its error stands
            const int32_t rec = A.out.cand_rec[ci] - A.recs.rec_base;
            if ((A.info[rec] & 255u) < IM_REC_ERR_RG) {
                if (A.out.rec_class) A.out.rec_class[rec] = (uint8_t)IM_REC_ERR_BASE;
                atomicAdd(&A.out.counters[3], 1);
            }
        }
    }
}

}  // namespace

// fixed words at the head of the scratch: chunk_base (256 B)
constexpr size_t kTriFixed = 256;

size_t triage_scratch_bytes(int32_t n_records)
{
    const size_t n = (size_t)(n_records > 0 ? n_records : 1);
    const size_t emits = (n + kTriBlock - 1) / kTriBlock;        // blk[]: one word per classify workgroup, whole emit workgroups; wg_base[]: one per emit workgroup
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    return up(n * 4) + up(n * 4) + up(emits * (kTriBlock / kClsBlock) * 8) + up(emits * 8) + up(n * 4) + kTriFixed;
}

// No word of the scratch has to hold anything before the first launch: every launch writes what it reads.  The entry point stays for
// the callers that have it; it clears the fixed words.
size_t triage_scratch_zero_offset(int32_t n_records, size_t* bytes)
{
    (void)n_records;
    *bytes = kTriFixed;
    return 0;
}

#ifdef IM_STAMPS
extern "C" int im_debug_tri_stamps_read(unsigned long long* out, int n_rec, int reset)
{
    if (n_rec < 0 || n_rec > kTriStampCap) return -1;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(im_tri_stamp_rec), (size_t)n_rec * 64);
    void* sym = nullptr;
    if (e == hipSuccess && reset) e = hipGetSymbolAddress(&sym, HIP_SYMBOL(im_tri_stamp_rec));
    if (e == hipSuccess && reset) e = hipMemset(sym, 0, sizeof(im_tri_stamp_rec));
    return e == hipSuccess ? 0 : -1;
}
#endif

hipError_t launch_triage(const RefDev& ref, const RgTable& rg, int32_t* depth_diff, const im_triage_params& tp,
                         const im_dev_records& recs, const im_dev_cands& out, void* scratch, hipStream_t stream)
{
    if (recs.n <= 0) return hipSuccess;
    const size_t n = (size_t)recs.n;
    const int blocks = (int)((n + kTriBlock - 1) / kTriBlock), cls_blocks = (int)((n + kClsBlock - 1) / kClsBlock);
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    TriageArgs A;
    A.recs = recs; A.out = out; A.tp = tp; A.ref = ref; A.rg = rg;
    A.depth_diff = tp.want_depth ? depth_diff : nullptr;
    // fixed words first (their place must not depend on the launch's record count), then the per-record arrays
    char* s = static_cast<char*>(scratch);
    A.chunk_base = reinterpret_cast<int32_t*>(s); s += 256;
    A.info = reinterpret_cast<uint32_t*>(s); s += up(n * 4);
    A.rmax = reinterpret_cast<int32_t*>(s); s += up(n * 4);
    A.blk = reinterpret_cast<uint2*>(s); s += up((size_t)blocks * (kTriBlock / kClsBlock) * 8);      // whole groups of kTriGroup words: up()'s 256 bytes
    A.wg_base = reinterpret_cast<uint2*>(s); s += up((size_t)blocks * 8);
    A.seq_at = reinterpret_cast<uint32_t*>(s);
    hipLaunchKernelGGL(triage_classify_kernel, dim3(cls_blocks), dim3(kClsBlock), 0, stream, A);
    hipLaunchKernelGGL(triage_scan_kernel, dim3(1), dim3(kScanLanes), 0, stream, A);
    hipLaunchKernelGGL(triage_emit_kernel, dim3(blocks), dim3(kTriBlock), 0, stream, A);
    int dgrid = (int)((n + 63) / 64);           // one 32-lane group per candidate, 8 per workgroup; ~1/8 of the records at most pays off
    if (dgrid > 16384) dgrid = 16384;           // a candidate per 32-lane group while that stays a sane grid: a group's candidates are a chain of dependent loads each
    hipLaunchKernelGGL(triage_decode_kernel, dim3(dgrid), dim3(256), 0, stream, A);
    return hipGetLastError();
}

}  // namespace im
