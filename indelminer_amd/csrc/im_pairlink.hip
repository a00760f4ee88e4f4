// im_pairlink.hip -- the read pairs whose orientation says "junction" (-M): kept in a keyed table of their own, counted between two
// windows (gfx950).  The definition is in include/indelminer_amd.h (seam 5, "Pair links"); DESIGN.md 4.5j has the cost.
//
// A delivered record that is the leftmost of a pair on one contig, both reads mapped, neither read in the normal orientation
// (forward in front of reverse), stores ONE LINK (tid, kind, pos, mpos): kind 0 EVERTED (this read reverse, its mate forward: a tandem
// duplication's pairs), 1 FORWARD (both forward: an inversion's left junction), 2 REVERSE (both reverse: its right junction).
//
// THE TABLE is the keyed table of im_keyed.hpp (slots, tickets, claim, walk), an allocation of its own, with
//   word 0   the key: bit 63 set (an empty slot is 0) | tid << 26 | (pos >> 8) << 2 | kind            (tid < 2^24, pos < 2^31)
//   word 1   the payload: pos | mpos << 32
// The whole key enters the hash: every link of one (tid, 256-base bucket, kind) lies on one probe run.
//
//   pairlink_scatter   one lane per delivered record; the lanes that hold a link insert it, on tickets their workgroup draws with one
//                      atomic add
//   pairlink_add       one lane per link, for callers that name the events themselves
//   pairlink_count     one wave per query (kind, a0, a1, b0, b1): the links with pos in [a0, a1], mpos in [b0, b1], mpos - pos >= min_sep

#include "im_keyed.hpp"
#include "im_rg.hpp"

namespace im {
namespace {

constexpr int kLinkBlock = 1024;      // records of a scatter workgroup: one ticket draw each
constexpr int kLinkWaveBlock = 256;   // threads of the add and count kernels
constexpr int kLinkBucketShift = 8;   // a bucket is 256 bases: a query window of 1 000 bases walks 4 or 5 probe runs

__device__ __forceinline__ uint64_t link_key(int32_t tid, int64_t bucket, uint32_t kind)
{
    return kKeyedUsed | ((uint64_t)(uint32_t)tid << 26) | ((uint64_t)bucket << 2) | kind;
}

__device__ __forceinline__ uint64_t link_payload(int64_t pos, int64_t mpos) { return (uint64_t)(uint32_t)pos | ((uint64_t)(uint32_t)mpos << 32); }

struct LinkScatterArgs {
    im_dev_records recs;
    const int32_t* len;
    int32_t n_contigs, min_mapq;
    KeyedTable tab;
};

// The record rule, on the 32-byte core alone.  Returns whether record i stores a link; *key, *payload: what it stores.
__device__ __forceinline__ bool link_of_record(const LinkScatterArgs& A, int64_t i, uint64_t* key, uint64_t* payload)
{
    if (i >= A.recs.n) return false;
    const RecView r = view_record(A.recs.raw, A.recs.rec_off[i], A.recs.rec_off[i + 1]);
    if (r.len < 32u) return false;
    if (!(r.flag & 0x1u) || (r.flag & (0x4u | 0x8u | 0x100u | 0x200u | 0x400u | 0x800u))) return false;
    if (r.tid < 0 || r.tid >= A.n_contigs || r.mtid != r.tid) return false;
    if (!(r.pos < r.mpos || (r.pos == r.mpos && (r.flag & 0x40u)))) return false;      // each pair once, at its leftmost record
    if ((int32_t)r.mapq < A.min_mapq) return false;
    const int32_t clen = A.len[r.tid];
    if (r.pos < 0 || r.pos > clen || r.mpos < 0 || r.mpos > clen) return false;
    const uint32_t rev = (r.flag >> 4) & 1u, mrev = (r.flag >> 5) & 1u;
    if (!rev && mrev) return false;                                 // the normal orientation is no link, whatever its insert size
    const uint32_t kind = rev ? (mrev ? 2u : 0u) : 1u;
    *key = link_key(r.tid, r.pos >> kLinkBucketShift, kind);
    *payload = link_payload(r.pos, r.mpos);
    return true;
}

// one ticket draw per workgroup (keyed_block_tickets has the reason); a workgroup without a link -- most of them -- ends there
__global__ __launch_bounds__(kLinkBlock) void pairlink_scatter_kernel(LinkScatterArgs A)
{
    uint64_t key = 0, payload = 0;
    const bool has = link_of_record(A, (int64_t)blockIdx.x * kLinkBlock + threadIdx.x, &key, &payload);
    unsigned long long ticket;
    if (!keyed_block_tickets<kLinkBlock, 1>(A.tab, has ? 1u : 0u, &ticket)) return;
    if (has && keyed_admit(A.tab, ticket)) keyed_place(A.tab, keyed_home(key, A.tab.log2_slots), key, payload);
}

// for callers that name the events themselves: one lane per link; positions outside [0, clen] are dropped (no ticket)
__global__ __launch_bounds__(kLinkWaveBlock) void pairlink_add_kernel(int32_t n, int32_t tid, int64_t clen, const int32_t* __restrict__ pos,
                                                                      const int32_t* __restrict__ mpos, const uint8_t* __restrict__ kind, KeyedTable tab)
{
    const int64_t i = (int64_t)blockIdx.x * kLinkWaveBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t p = pos[i], m = mpos[i];
    if (p < 0 || p > clen || m < 0 || m > clen) return;
    const uint64_t key = link_key(tid, p >> kLinkBucketShift, kind[i]);
    keyed_insert(tab, keyed_home(key, tab.log2_slots), key, link_payload(p, m));
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

// One wave per query.  Both intervals are clipped to [0, clen]; for every bucket of the pos interval (at most 257: the caller holds
// a1 - a0 to 65 535) the wave walks the bucket's probe run (keyed_walk).  A lane's slot counts when its key is the bucket's and its
// payload passes the three tests; the wave sums by ballot and popcount.  Every branch is on values the whole wave shares; both loops
// are bounded, by the bucket count and the slot count.
__global__ __launch_bounds__(kLinkWaveBlock) void pairlink_count_kernel(LinkCountArgs A)
{
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int q = wave; q < A.nq; q += nwaves) {
        int64_t a0 = A.a0[q], a1 = A.a1[q], b0 = A.b0[q], b1 = A.b1[q];
        const uint32_t kind = A.kind[q];
        a0 = a0 < 0 ? 0 : a0; b0 = b0 < 0 ? 0 : b0;
        a1 = a1 > A.clen ? A.clen : a1; b1 = b1 > A.clen ? A.clen : b1;
        uint32_t n = 0;
        if (a0 <= a1 && b0 <= b1) {
            for (int64_t bucket = a0 >> kLinkBucketShift; bucket <= (a1 >> kLinkBucketShift); bucket++) {
                const uint64_t want = link_key(A.tid, bucket, kind);
                (void)keyed_walk(A.tab, keyed_home(want, A.tab.log2_slots), [want](uint64_t key) { return key == want; }, lane,
                                 [&](bool has, uint64_t, uint64_t s) {
                    bool counts = false;
                    if (has) {
                        const uint64_t payload = A.tab.slots[2ull * s + 1ull];
                        const int64_t pos = (int64_t)(uint32_t)payload, mpos = (int64_t)(uint32_t)(payload >> 32);
                        counts = pos >= a0 && pos <= a1 && mpos >= b0 && mpos <= b1 && mpos - pos >= (int64_t)A.min_sep;
                    }
                    n += (uint32_t)__builtin_popcountll(__ballot(counts));
                });
            }
        }
        if (lane == 0) A.count[q] = n;
    }
}

}  // namespace

hipError_t launch_pairlink_scatter(const RefDev& ref, int32_t min_mapq, const im_dev_records& recs, const KeyedTable& tab, hipStream_t stream)
{
    if (recs.n <= 0) return hipSuccess;
    LinkScatterArgs A;
    A.recs = recs; A.len = ref.len; A.n_contigs = ref.n_contigs; A.min_mapq = min_mapq; A.tab = tab;
    hipLaunchKernelGGL(pairlink_scatter_kernel, dim3((recs.n + kLinkBlock - 1) / kLinkBlock), dim3(kLinkBlock), 0, stream, A);
    return hipGetLastError();
}

hipError_t launch_pairlink_add(int32_t n, int32_t tid, int64_t clen, const int32_t* pos, const int32_t* mpos, const uint8_t* kind,
                               const KeyedTable& tab, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pairlink_add_kernel, dim3((n + kLinkWaveBlock - 1) / kLinkWaveBlock), dim3(kLinkWaveBlock), 0, stream, n, tid, clen, pos, mpos, kind, tab);
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

}  // namespace im
