// im_matelink.hip -- the read pairs whose mate lies on ANOTHER contig (-T): kept in a keyed table of their own, asked where the mates
// of the reads around a position lie (gfx950).  The definition is in include/indelminer_amd.h (seam 5, "Mate links"); DESIGN.md 4.5k
// has the cost.
//
// A delivered record that is paired, both reads mapped, its mate on another contig, stores ONE LINK (tid, kind, pos, mtid, mpos) at its
// own contig: kind = r | m << 1, r = this read reverse, m = its mate reverse.  Both reads of a pair store one each.
//
// THE TABLE is the keyed table of im_keyed.hpp (slots, tickets, claim, walk), an allocation of its own, with
//   word 0   the key: bit 63 set (an empty slot is 0) | tid << 26 | (pos >> 8) << 2 | kind            (tid < 2^24, pos < 2^31)
//   word 1   the payload: pos & 255 | mtid << 8 | mpos << 32
// The whole key enters the hash: every link of one (tid, 256-base bucket, kind) lies on one probe run -- the pair links' bucket rule.
//
//   matelink_scatter   one lane per delivered record; the lanes that hold a link insert it, on tickets their workgroup draws with one
//                      atomic add
//   matelink_add       one lane per link, for callers that name the events themselves
//   matelink_partner   one wave per query (kind, a0, a1): the links with pos in [a0, a1] vote for the cell (mtid, mpos >> 10) of their
//                      mate in a table in LDS; the pair of neighbouring cells with the most links wins

#include "im_keyed.hpp"
#include "im_rg.hpp"
#include "im_wave.hpp"

namespace im {
namespace {

constexpr int kMateBlock = 1024;      // records of a scatter workgroup: one ticket draw each
constexpr int kMateWaveBlock = 256;   // threads of the add and partner kernels
constexpr int kMateBucketShift = 8;   // a bucket is 256 bases, as the pair links'
constexpr int kMateCellShift = 10;    // a cell is 1 024 bases of the mate's contig
constexpr int kMateCells = IM_MATELINK_CELLS;
static_assert(kMateCells == 256, "a cell's slot is the top 8 bits of its hash, and a lane owns kMateCells / 64 slots");

__device__ __forceinline__ uint64_t mate_key(int32_t tid, int64_t bucket, uint32_t kind)
{
    return kKeyedUsed | ((uint64_t)(uint32_t)tid << 26) | ((uint64_t)bucket << 2) | kind;
}

__device__ __forceinline__ uint64_t mate_payload(int64_t pos, int32_t mtid, int64_t mpos)
{
    return (uint64_t)((uint32_t)pos & 255u) | ((uint64_t)(uint32_t)mtid << 8) | ((uint64_t)(uint32_t)mpos << 32);
}

struct MateScatterArgs {
    im_dev_records recs;
    const int32_t* len;
    int32_t n_contigs, min_mapq;
    KeyedTable tab;
};

// The record rule, on the 32-byte core alone.  Returns whether record i stores a link; *key, *payload: what it stores.
__device__ __forceinline__ bool mate_of_record(const MateScatterArgs& A, int64_t i, uint64_t* key, uint64_t* payload)
{
    if (i >= A.recs.n) return false;
    const RecView r = view_record(A.recs.raw, A.recs.rec_off[i], A.recs.rec_off[i + 1]);
    if (r.len < 32u) return false;
    if (!(r.flag & 0x1u) || (r.flag & (0x4u | 0x8u | 0x100u | 0x200u | 0x400u | 0x800u))) return false;
    if (r.tid < 0 || r.tid >= A.n_contigs || r.mtid < 0 || r.mtid >= A.n_contigs || r.mtid == r.tid) return false;
    if ((int32_t)r.mapq < A.min_mapq) return false;
    if (r.pos < 0 || r.pos > A.len[r.tid] || r.mpos < 0 || r.mpos > A.len[r.mtid]) return false;
    const uint32_t kind = ((r.flag >> 4) & 1u) | (((r.flag >> 5) & 1u) << 1);
    *key = mate_key(r.tid, r.pos >> kMateBucketShift, kind);
    *payload = mate_payload(r.pos, r.mtid, r.mpos);
    return true;
}

// one ticket draw per workgroup (keyed_block_tickets has the reason); a workgroup without a link -- most of them -- ends there
__global__ __launch_bounds__(kMateBlock) void matelink_scatter_kernel(MateScatterArgs A)
{
    uint64_t key = 0, payload = 0;
    const bool has = mate_of_record(A, (int64_t)blockIdx.x * kMateBlock + threadIdx.x, &key, &payload);
    unsigned long long ticket;
    if (!keyed_block_tickets<kMateBlock, 1>(A.tab, has ? 1u : 0u, &ticket)) return;
    if (has && keyed_admit(A.tab, ticket)) keyed_place(A.tab, keyed_home(key, A.tab.log2_slots), key, payload);
}

// for callers that name the events themselves: one lane per link; a link that fails the rule's range checks is dropped (no ticket)
__global__ __launch_bounds__(kMateWaveBlock) void matelink_add_kernel(int32_t n, int32_t tid, const int32_t* __restrict__ len, int32_t n_contigs,
                                                                      const int32_t* __restrict__ pos, const int32_t* __restrict__ mtid,
                                                                      const int32_t* __restrict__ mpos, const uint8_t* __restrict__ kind, KeyedTable tab)
{
    const int64_t i = (int64_t)blockIdx.x * kMateWaveBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pos[i], m = mpos[i];
    const int32_t mt = mtid[i];
    if (mt < 0 || mt >= n_contigs || mt == tid) return;
    if (p < 0 || p > len[tid] || m < 0 || m > len[mt]) return;
    const uint64_t key = mate_key(tid, p >> kMateBucketShift, kind[i]);
    keyed_insert(tab, keyed_home(key, tab.log2_slots), key, mate_payload(p, mt, m));
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

// One wave per query.  The interval is clipped to [0, clen]; for every bucket of it (at most 257: the caller holds a1 - a0 to 65 535)
// the wave walks the bucket's probe run (keyed_walk).  A lane whose slot holds a link of the interval claims the link's cell in the
// wave's LDS table with a 64-bit compare-and-swap and adds the link to the cell's count, minimum and maximum with LDS atomics: sums,
// minima and maxima, so nothing depends on the order of arrival, and a cell finds no slot only when 256 others hold them all.  Then
// every lane takes four slots: an occupied one looks up its right neighbour, its score is the two counts, and the wave reduces
// (score, the smallest cell key among equals -- mtid in the high word, the cell in the low one).  A cell (mtid, c) that holds no link
// while (mtid, c + 1) does need not stand: its links are those of (mtid, c + 1) or fewer, and the answer names links, not c.  Every
// branch is on values the whole wave shares; every loop is bounded, by the bucket count, the slot count or kMateCells.  The LDS one
// lane writes and another reads is ordered by wave_lds_sync (im_wave.hpp): LDS executes a wave's instructions in order.
__global__ __launch_bounds__(kMateWaveBlock) void matelink_partner_kernel(MatePartnerArgs A)
{
    __shared__ MateCellTable s_cells[kMateWaveBlock / 64];
    const int lane = threadIdx.x & 63;
    MateCellTable& C = s_cells[threadIdx.x >> 6];
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < A.nq; q += nwaves) {
        int64_t a0 = A.a0[q], a1 = A.a1[q];
        const uint32_t kind = A.kind[q];
        a0 = a0 < 0 ? 0 : a0;
        a1 = a1 > A.clen ? A.clen : a1;
#pragma unroll
        for (int j = 0; j < kMateCells / 64; j++) {
            const int s = lane + 64 * j;
            C.key[s] = 0ull; C.cnt[s] = 0u; C.lo[s] = 0xFFFFFFFFu; C.hi[s] = 0u;
        }
        wave_lds_sync();
        uint32_t n = 0;
        bool over = false;
        if (a0 <= a1) {
            for (int64_t bucket = a0 >> kMateBucketShift; bucket <= (a1 >> kMateBucketShift); bucket++) {
                const uint64_t want = mate_key(A.tid, bucket, kind);
                (void)keyed_walk(A.tab, keyed_home(want, A.tab.log2_slots), [want](uint64_t key) { return key == want; }, lane,
                                 [&](bool has, uint64_t, uint64_t s) {
                    const uint64_t payload = has ? A.tab.slots[2ull * s + 1ull] : 0ull;
                    const int64_t pos = (bucket << kMateBucketShift) | (int64_t)(payload & 255ull);
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
            }
        }
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

}  // namespace

hipError_t launch_matelink_scatter(const RefDev& ref, int32_t min_mapq, const im_dev_records& recs, const KeyedTable& tab, hipStream_t stream)
{
    if (recs.n <= 0) return hipSuccess;
    MateScatterArgs A;
    A.recs = recs; A.len = ref.len; A.n_contigs = ref.n_contigs; A.min_mapq = min_mapq; A.tab = tab;
    hipLaunchKernelGGL(matelink_scatter_kernel, dim3((recs.n + kMateBlock - 1) / kMateBlock), dim3(kMateBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_matelink_add(const RefDev& ref, int32_t n, int32_t tid, const int32_t* pos, const int32_t* mtid, const int32_t* mpos,
                               const uint8_t* kind, const KeyedTable& tab, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(matelink_add_kernel, dim3((n + kMateWaveBlock - 1) / kMateWaveBlock), dim3(kMateWaveBlock), 0, stream, n, tid, ref.len, ref.n_contigs,
                       pos, mtid, mpos, kind, tab);
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
    hipLaunchKernelGGL(matelink_partner_kernel, dim3(wave_grid(nq)), dim3(kMateWaveBlock), 0, stream, A);
    return hipGetLastError();
}

}  // namespace im
