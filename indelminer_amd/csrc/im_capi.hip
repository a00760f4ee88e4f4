// im_capi.hip -- the C ABI of include/indelminer_amd.h over the HIP kernels.
// No CPU fallback anywhere: without a gfx950 device every entry point fails.

#include "im_device.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>
#include <unordered_map>
#include <mutex>
#include <atomic>

// One contig's difference array of the record-at-a-time path (im_depth_build, im_span_build, im_pairspan_build): cap ints of data and the sums
// im::depth_sums_ints gives for cap - 1 positions (it grows with the contig, so they serve every shorter one); len < 0: not built
struct ContigArray {
    int32_t* data = nullptr;
    int32_t* sums = nullptr;
    int64_t cap = 0, len = -1;
};

// One genome-wide array of that layout (im_depth_enable, im_span_enable, im_pairspan_enable): one int32 per byte of ref_ascii and every contig's own run
// of tile sums, allocated on that call only; flank and min_mapq are what its scatter counts by (the depth array has neither)
struct GenomeArray {
    int32_t* data = nullptr;
    int32_t* sums = nullptr;
    int32_t flank = 0, min_mapq = 0;
};

// One keyed table (im_keyed.hpp) with what its scatter counts by (min_clip: the clip tails'; 0 elsewhere) and the entry point that
// enables it, for the messages; slots null: not enabled
struct KeyedMember : im::KeyedTable {
    const char* enable;
    int32_t min_clip = 0, min_mapq = 0;
    explicit KeyedMember(const char* enable_) : im::KeyedTable{nullptr, nullptr, 0}, enable(enable_) {}
};

struct im_ctx {
    int device = -1;
    int n_cu = 0;
    std::atomic<int> expect_len{0};     // im_expect_read_length: beyond kShortRead the long-read pass follows every realign launch
    hipStream_t stream = nullptr;
    char err[512] = {0};
    // reference
    int32_t n_contigs = 0;
    uint8_t* ref_ascii = nullptr;
    uint64_t* ref_pk = nullptr;
    int64_t* d_asc_off = nullptr;
    int64_t* d_pk_off = nullptr;
    int32_t* d_len = nullptr;
    // reusable device workspace for the host-buffer entry points
    void* ws = nullptr;
    size_t ws_bytes = 0;
    // pinned host staging of the host-buffer entry points, and a second stream for their copies
    void* pin = nullptr;
    size_t pin_bytes = 0;
    hipStream_t copy_stream = nullptr, back_stream = nullptr;     // host -> device, device -> host
    hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr}, ev_out[2] = {nullptr, nullptr};
    // resident depth, span and pair-span arrays of the current contig (im_depth_build, im_span_build, im_pairspan_build)
    ContigArray depth, span, pair;
    // -C: the clipped-read counts of the current contig, right and left (im_clip_build); point counts, no sums
    ContigArray clip_r, clip_l;
    // host copies of the reference layout
    std::vector<int64_t> h_asc_off;
    std::vector<int32_t> h_len;
    int64_t ref_total = 0;
    // genome-wide depth / difference array, reference-spanning counts and concordant-pair counts
    GenomeArray all_depth, all_span, all_pair;
    // genome-wide clipped-read counts, right and left (im_clip_enable): flank holds min_clip; never scanned, their sums stay null
    GenomeArray all_clip_r, all_clip_l;
    // the keyed tables, an allocation each: -V the clipped bases, -M the pair links, -T the mate links, -S the split links
    KeyedMember tail{"im_cliptail_enable"}, link{"im_pairlink_enable"}, mate{"im_matelink_enable"}, split{"im_splitlink_enable"};
    // the contig names im_splitlink_enable was given, and their blob on the device (im_links.hip has the layout)
    std::vector<std::string> split_names;
    uint8_t* split_blob = nullptr;
    // -H: the overlap of every stored split link, a 16-bit code per slot of the split table (im_splitlink_overlap_enable); null: off
    uint16_t* split_ovl = nullptr;
    // -E: the pair-link table also takes kind 3, the stretched pairs (im_pairlink_stretched_enable); goes with the table
    bool link_stretched = false;
    // the median queries' histograms of queries of several slabs (im::launch_depth_median): zeros between calls, sized by the call that
    // needed the most; med_dirty: a call did not get to its end, the next one clears them
    uint32_t* med_scratch = nullptr;
    int32_t med_slots = 0;
    bool med_dirty = false;
    bool support_count_attr = false;    // im_support_count: its kernel's LDS attribute has been set on this context's device
    std::mutex gb_mu;
    std::unordered_map<void*, int32_t> gb_layout;   // group-by scratch -> the slot count it was initialised (and is carved) for
    std::unordered_map<void*, std::pair<int32_t, int32_t>> fg_layout;   // flush + group-by scratch -> (slots, flushes) it is carved for
    std::vector<int64_t> h_sums_off;    // each contig's own run of tile sums: scans of different contigs may be in flight on different streams
    // read-group -> range[1] table (im_set_insert_ranges), flattened hashtable chains
    void* rg_blob = nullptr;
    im::RgTable rg = {nullptr, 0, 0, 0, 0};
    // the general realign pass (im_realign_any.hip): list of the reads it takes, counters, arena; one call at a time
    std::mutex any_mu;
    int32_t* any_list = nullptr; int32_t any_list_cap = 0;
    int32_t* any_counters = nullptr;
    int32_t* any_arena = nullptr; size_t any_arena_bytes = 0;
};

namespace {

char g_err[512] = "";

void set_err(im_ctx* ctx, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    char* dst = ctx ? ctx->err : g_err;
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
}

#define HIP_TRY(ctx, expr)                                                              \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            set_err(ctx, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return IM_E_HIP;                                                            \
        }                                                                               \
    } while (0)

int check_params(im_ctx* ctx, const im_params* p)
{
    if (!p) { set_err(ctx, "params is NULL"); return IM_E_ARG; }
    // forceassert((klength > 1) && (klength < 16)), src/indelminer.c:1028
    if (p->klength < 2 || p->klength > 15) { set_err(ctx, "klength %u outside 2..15", p->klength); return IM_E_ARG; }
    if (p->maxdelsize == 0) { set_err(ctx, "maxdelsize must be > 0"); return IM_E_ARG; }
    if (p->numgaps > (1u << 20)) { set_err(ctx, "numgaps=%u", p->numgaps); return IM_E_ARG; }
    return IM_OK;
}

int ensure_ws(im_ctx* ctx, size_t bytes)
{
    if (bytes <= ctx->ws_bytes) return IM_OK;
    if (ctx->ws) { HIP_TRY(ctx, hipFree(ctx->ws)); ctx->ws = nullptr; ctx->ws_bytes = 0; }
    bytes = (bytes + (1u << 20) - 1) / (1u << 20) * (1u << 20);
    HIP_TRY(ctx, hipMalloc(&ctx->ws, bytes));
    ctx->ws_bytes = bytes;
    return IM_OK;
}

int ensure_pin(im_ctx* ctx, size_t bytes)
{
    if (bytes <= ctx->pin_bytes) return IM_OK;
    if (ctx->pin) { HIP_TRY(ctx, hipHostFree(ctx->pin)); ctx->pin = nullptr; ctx->pin_bytes = 0; }
    bytes = (bytes + (1u << 20) - 1) / (1u << 20) * (1u << 20);
    HIP_TRY(ctx, hipHostMalloc(&ctx->pin, bytes, hipHostMallocDefault));
    ctx->pin_bytes = bytes;
    return IM_OK;
}

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

void free_reference(im_ctx* ctx)
{
    if (ctx->ref_ascii) (void)hipFree(ctx->ref_ascii);
    if (ctx->ref_pk) (void)hipFree(ctx->ref_pk);
    if (ctx->d_asc_off) (void)hipFree(ctx->d_asc_off);
    if (ctx->d_pk_off) (void)hipFree(ctx->d_pk_off);
    if (ctx->d_len) (void)hipFree(ctx->d_len);
    ctx->ref_ascii = nullptr; ctx->ref_pk = nullptr; ctx->d_asc_off = nullptr; ctx->d_pk_off = nullptr; ctx->d_len = nullptr;
    ctx->n_contigs = 0;
    for (GenomeArray* g : {&ctx->all_depth, &ctx->all_span, &ctx->all_pair, &ctx->all_clip_r, &ctx->all_clip_l}) {
        if (g->data) (void)hipFree(g->data);
        if (g->sums) (void)hipFree(g->sums);
        g->data = nullptr; g->sums = nullptr;
    }
    ctx->h_asc_off.clear(); ctx->h_len.clear(); ctx->ref_total = 0;
    // the clip-tail table and the three link tables are keyed by the contigs of the reference that goes
    for (KeyedMember* t : {&ctx->tail, &ctx->link, &ctx->mate, &ctx->split}) {
        if (t->slots) (void)hipFree(t->slots);
        if (t->counters) (void)hipFree(t->counters);
        *t = KeyedMember(t->enable);
    }
    if (ctx->split_blob) (void)hipFree(ctx->split_blob);
    ctx->split_blob = nullptr; ctx->split_names.clear();
    if (ctx->split_ovl) (void)hipFree(ctx->split_ovl);
    ctx->split_ovl = nullptr;
    ctx->link_stretched = false;
}

// ---- the keyed table (im_keyed.hpp) behind the clip tails (im_ctx::tail), the pair links (im_ctx::link), the mate links (im_ctx::mate) and the split links (im_ctx::split) ----------

// An enable call from its first check to its last.  min_clip: null for the families that have none.  A member that is enabled already
// takes the same parameters again and no others; otherwise its slots and counters are allocated, cleared and waited for.
int keyed_enable(im_ctx* ctx, KeyedMember im_ctx::*which, const int32_t* min_clip, int32_t min_mapq, int32_t log2_slots)
{
    if (!ctx) return IM_E_ARG;
    KeyedMember& T = ctx->*which;
    if (!ctx->ref_ascii) { set_err(ctx, "im_set_reference has not been called"); return IM_E_ARG; }
    if (min_clip && *min_clip < 1) { set_err(ctx, "%s: min_clip %d, must be >= 1", T.enable, *min_clip); return IM_E_ARG; }
    if (log2_slots < 6 || log2_slots > 30) { set_err(ctx, "%s: log2_slots %d, must be 6 .. 30", T.enable, log2_slots); return IM_E_ARG; }
    if (ctx->n_contigs > (1 << 24)) { set_err(ctx, "%s: more than 2^24 contigs", T.enable); return IM_E_ARG; }
    const int32_t clip = min_clip ? *min_clip : 0;
    if (T.slots) {
        if (clip == T.min_clip && min_mapq == T.min_mapq && log2_slots == T.log2_slots) return IM_OK;
        char clipped[32] = "";
        if (min_clip) snprintf(clipped, sizeof clipped, "min_clip %d, ", T.min_clip);
        set_err(ctx, "%s: already enabled with %smin_mapq %d, log2_slots %d", T.enable, clipped, T.min_mapq, T.log2_slots);
        return IM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)16 << log2_slots;
    unsigned long long* slots = nullptr;
    unsigned long long* counters = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&slots, bytes));
    if (hipMalloc((void**)&counters, 2 * sizeof(unsigned long long)) != hipSuccess) { (void)hipFree(slots); set_err(ctx, "%s: out of device memory", T.enable); return IM_E_HIP; }
    T.slots = slots; T.counters = counters; T.log2_slots = log2_slots; T.min_clip = clip; T.min_mapq = min_mapq;
    HIP_TRY(ctx, hipMemsetAsync(slots, 0, bytes, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return IM_OK;
}

// What every other entry point asks first: the table enabled and, where the call names one (tid non-null), a contig of the reference
int keyed_ready(im_ctx* ctx, const KeyedMember& T, const int32_t* tid)
{
    if (!T.slots) { set_err(ctx, "%s has not been called", T.enable); return IM_E_ARG; }
    if (tid && (*tid < 0 || *tid >= ctx->n_contigs)) return IM_E_ARG;
    return IM_OK;
}

int keyed_reset(im_ctx* ctx, KeyedMember im_ctx::*which, void* stream)
{
    if (!ctx || !(ctx->*which).slots) return IM_E_ARG;
    const im::KeyedTable& T = ctx->*which;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(T.slots, 0, (size_t)16 << T.log2_slots, (hipStream_t)stream));
    HIP_TRY(ctx, hipMemsetAsync(T.counters, 0, 2 * sizeof(unsigned long long), (hipStream_t)stream));
    return IM_OK;
}

// the two counters, copied on the context's stream behind what the caller has queued there, and the ONE wait of its call
int keyed_counters(im_ctx* ctx, const im::KeyedTable& T, unsigned long long counters[2])
{
    HIP_TRY(ctx, hipMemcpyAsync(counters, T.counters, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return IM_OK;
}

// the same, for a query: whether the table has dropped an entry, so that the caller blanks its answers -- none, not a wrong one
int keyed_overflowed(im_ctx* ctx, const im::KeyedTable& T, bool* over)
{
    unsigned long long counters[2] = {0, 0};
    const int rc = keyed_counters(ctx, T, counters);
    *over = counters[1] > 0;
    return rc;
}

int keyed_stats(im_ctx* ctx, KeyedMember im_ctx::*which, uint64_t* stored, uint64_t* dropped)
{
    if (!ctx || !(ctx->*which).slots || !stored || !dropped) return IM_E_ARG;
    const im::KeyedTable& T = ctx->*which;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long counters[2] = {0, 0};
    const int rc = keyed_counters(ctx, T, counters);
    if (rc) return rc;
    const unsigned long long half = 1ull << (T.log2_slots - 1);
    *stored = counters[0] < half ? counters[0] : half; *dropped = counters[1];
    return IM_OK;
}

// The workspace as columns of n elements for the entry points of the four tables: column k at k * up256(4 n) bytes (a column of 8-byte
// elements takes two), host -> device and back on the context's stream.
struct WsColumns {
    im_ctx* ctx;
    size_t n, sb;
    template <class T> T* at(int k) const { return (T*)((char*)ctx->ws + k * sb); }
    int down(int k, const void* host, size_t elem) const { HIP_TRY(ctx, hipMemcpyAsync(at<char>(k), host, elem * n, hipMemcpyHostToDevice, ctx->stream)); return IM_OK; }
    int up(int k, void* host, size_t elem) const { HIP_TRY(ctx, hipMemcpyAsync(host, at<char>(k), elem * n, hipMemcpyDeviceToHost, ctx->stream)); return IM_OK; }
};

int ws_columns(im_ctx* ctx, int32_t n, int k, WsColumns* C)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *C = {ctx, (size_t)n, up256(sizeof(int32_t) * (size_t)n)};
    return ensure_ws(ctx, k * C->sb);
}

// The end of a query: its answers, in columns from `first` on (one of 8-byte elements takes two), up to the host behind the launch, the
// table's counters with them and the ONE wait; after an overflow every answer is 0xFF bytes -- "none", not a wrong one
struct Answer { void* host; size_t elem; };

int keyed_answers(im_ctx* ctx, const im::KeyedTable& T, const WsColumns& C, int first, std::initializer_list<Answer> answers)
{
    int rc = IM_OK, k = first;
    for (const Answer& a : answers) {
        if ((rc = C.up(k, a.host, a.elem))) return rc;
        k += a.elem > 4 ? 2 : 1;
    }
    bool over = false;
    if ((rc = keyed_overflowed(ctx, T, &over))) return rc;
    if (over) for (const Answer& a : answers) memset(a.host, 0xFF, a.elem * C.n);
    return IM_OK;
}

// What the add and query calls of both link families check per link or query (what: "link", "query"): its kind, and -- a0 non-null --
// that the wave walks 257 buckets at the most, one probe run per 256-base bucket of [a0, a1]
struct LinkKinds { uint8_t max; const char* words; };
constexpr LinkKinds kPairKinds = {2, "0 (everted), 1 (forward) or 2 (reverse)"}, kPairKindsStretched = {3, "0 (everted), 1 (forward), 2 (reverse) or 3 (stretched)"}, kMateKinds = {3, "0 .. 3 (read reverse | mate reverse << 1)"};

int link_args(im_ctx* ctx, const char* who, const char* what, const LinkKinds& K, int32_t n, const uint8_t* kind, const int32_t* a0, const int32_t* a1)
{
    for (int32_t i = 0; i < n; i++) {
        if (kind[i] > K.max) { set_err(ctx, "%s: %s %d: kind %d, must be %s", who, what, i, (int)kind[i], K.words); return IM_E_ARG; }
        const long long span = a0 ? (long long)a1[i] - (long long)a0[i] : 0;
        if (span > 65535) { set_err(ctx, "%s: %s %d: a1 - a0 = %lld, must be <= 65535", who, what, i, span); return IM_E_ARG; }
    }
    return IM_OK;
}

void free_array(ContigArray& a)
{
    if (a.data) (void)hipFree(a.data);
    if (a.sums) (void)hipFree(a.sums);
    a = ContigArray();
}

// The helpers below serve one member of either family each; `family` ("im_depth", "im_span", "im_pairspan") names it in the messages, and
// flank is null for the depth arrays, which count whole intervals.

// a build's first step: the array counts as not built until the build is through, and holds clen + 1 entries (with_sums: and its tile sums)
int grow_array(im_ctx* ctx, ContigArray& a, int64_t clen, bool with_sums)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    a.len = -1;
    if (clen + 1 > a.cap) {
        free_array(a);
        HIP_TRY(ctx, hipMalloc((void**)&a.data, (size_t)(clen + 1) * sizeof(int32_t)));
        if (with_sums) HIP_TRY(ctx, hipMalloc((void**)&a.sums, (size_t)im::depth_sums_ints(clen) * sizeof(int32_t)));     // zeroed by every build
        a.cap = clen + 1;
    }
    return IM_OK;
}

// im_depth_build / im_span_build / im_pairspan_build: check, grow, stage the intervals, memset + scatter + scan (one launcher, im_depth.hip), wait
int build_array(im_ctx* ctx, ContigArray im_ctx::*which, const char* family, int64_t clen, int32_t n, const int32_t* start, const int32_t* len,
                const int32_t* flank)
{
    if (!ctx || clen < 0 || clen > 0x7fffff00LL || n < 0 || (n > 0 && (!start || !len))) return IM_E_ARG;
    if (flank && *flank < 1) { set_err(ctx, "%s_build: flank %d, must be >= 1", family, *flank); return IM_E_ARG; }
    const int32_t lo = flank ? *flank : 0, hi = flank ? *flank - 1 : 0;
    ContigArray& a = ctx->*which;
    int rc = grow_array(ctx, a, clen, true);
    if (rc) return rc;
    const size_t sb = up256(sizeof(int32_t) * (size_t)(n ? n : 1));
    rc = ensure_ws(ctx, 2 * sb);
    if (rc) return rc;
    int32_t* d_start = (int32_t*)ctx->ws;
    int32_t* d_len = (int32_t*)((char*)ctx->ws + sb);
    if (n > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(d_start, start, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_len, len, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, im::launch_depth_build(clen, n, d_start, d_len, lo, hi, a.data, a.sums, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    a.len = clen;
    return IM_OK;
}

// what a query answers per interval: the sum over [beg, end) (the depth query; max_out, where not null, the deepest position of
// [beg - 1, end]), the minimum over [beg, end] (the span queries), or the lower median over [beg, end) of the values capped at 4095
// kArgMax: the largest value over [beg, end] and the smallest position that holds it, of one of two unscanned arrays (the clip queries)
enum Reduce { kSum, kMinimum, kMedian, kArgMax };

// what an arg-max query has beyond the family's (beg, end, out): per query which of the two arrays it reads (0: the helper's own,
// the right clips; 1: `other`, the left clips), and where the positions go
struct ArgMaxSide {
    const uint8_t* side;
    const int32_t* other;
    int32_t* pos_out;
};

// the median's trip, n > 0: [beg][end][first][slot] in, one launch (one per kMedMaxSlots queries of several slabs), out back, one wait.
// The answers of queries that are empty after the clip are set here.  The call that needs more histograms than any before it
// pays for them here (free, allocate, clear: at most 16 MB), under whatever lock the caller holds around its queries.
int median_array(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, const int32_t* data, const int32_t* sums, int64_t clen,
                 uint32_t* out)
{
    constexpr int32_t kMedMaxSlots = 1024;                  // 16 MB of histograms at the most
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<int32_t> first((size_t)n + 1), slot((size_t)n, -1), cut;      // cut: the queries at which a launch starts
    int64_t items = 0;
    int32_t used = 0, most = 0;
    cut.push_back(0);
    for (int32_t q = 0; q < n; q++) {
        const int32_t s = im::depth_median_slabs(beg[q], end[q], clen);
        first[q] = (int32_t)items;
        items += s;
        if (items > 0x7fffffff) { set_err(ctx, "median query: more than 2^31 slabs in one call"); return IM_E_ARG; }
        if (s > 1) {
            if (used == kMedMaxSlots) { cut.push_back(q); used = 0; }
            slot[q] = used++;
            if (used > most) most = used;
        }
    }
    first[n] = (int32_t)items;
    cut.push_back(n);
    if (most > ctx->med_slots) {
        if (ctx->med_scratch) { HIP_TRY(ctx, hipFree(ctx->med_scratch)); ctx->med_scratch = nullptr; ctx->med_slots = 0; }
        HIP_TRY(ctx, hipMalloc((void**)&ctx->med_scratch, im::depth_median_scratch_bytes(most)));
        ctx->med_slots = most;
        ctx->med_dirty = true;
    }
    if (ctx->med_dirty && ctx->med_scratch) HIP_TRY(ctx, hipMemsetAsync(ctx->med_scratch, 0, im::depth_median_scratch_bytes(ctx->med_slots), ctx->stream));
    const size_t sb = up256(sizeof(int32_t) * ((size_t)n + 1));
    int rc = ensure_ws(ctx, 5 * sb);
    if (rc) return rc;
    int32_t* d_beg = (int32_t*)ctx->ws;
    int32_t* d_end = (int32_t*)((char*)ctx->ws + sb);
    int32_t* d_first = (int32_t*)((char*)ctx->ws + 2 * sb);
    int32_t* d_slot = (int32_t*)((char*)ctx->ws + 3 * sb);
    uint32_t* d_out = (uint32_t*)((char*)ctx->ws + 4 * sb);
    if (items > 0) {
        ctx->med_dirty = true;
        HIP_TRY(ctx, hipMemcpyAsync(d_beg, beg, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_end, end, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_first, first.data(), sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_slot, slot.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        for (size_t k = 0; k + 1 < cut.size(); k++) {
            const int32_t q0 = cut[k], q1 = cut[k + 1];
            HIP_TRY(ctx, im::launch_depth_median(q1 - q0, first[q1] - first[q0], d_beg + q0, d_end + q0, d_first + q0, d_slot + q0, data, sums, clen,
                                                 ctx->med_scratch, ctx->med_slots, 8 * (ctx->n_cu > 0 ? ctx->n_cu : 256), d_out + q0, ctx->stream));
        }
        HIP_TRY(ctx, hipMemcpyAsync(out, d_out, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->med_dirty = false;
    for (int32_t q = 0; q < n; q++) if (first[q + 1] == first[q]) out[q] = 0xFFFFFFFFu;
    return IM_OK;
}

// the arg-max's trip, n > 0: [side][beg][end] in, one launch on the two arrays as they stand, counts and positions back, one wait
int argmax_array(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, const int32_t* data, int64_t clen, const ArgMaxSide& x, uint32_t* out)
{
    if (!x.side || !x.pos_out) return IM_E_ARG;
    for (int32_t q = 0; q < n; q++) if (x.side[q] > 1) { set_err(ctx, "clip query %d: side %d, must be 0 (right) or 1 (left)", q, (int)x.side[q]); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t sb = up256(sizeof(int32_t) * (size_t)n);
    int rc = ensure_ws(ctx, 5 * sb);
    if (rc) return rc;
    int32_t* d_beg = (int32_t*)ctx->ws;
    int32_t* d_end = (int32_t*)((char*)ctx->ws + sb);
    uint32_t* d_out = (uint32_t*)((char*)ctx->ws + 2 * sb);
    int32_t* d_pos = (int32_t*)((char*)ctx->ws + 3 * sb);
    uint8_t* d_side = (uint8_t*)ctx->ws + 4 * sb;
    HIP_TRY(ctx, hipMemcpyAsync(d_beg, beg, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_end, end, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_side, x.side, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, im::launch_clip_argmax(n, d_side, d_beg, d_end, data, x.other, clen, d_out, d_pos, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(x.pos_out, d_pos, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return IM_OK;
}

// the queries' trip through the context's workspace and stream, n > 0: [beg][end] in, one launch on a scanned array, out back
int query_array(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, const int32_t* data, const int32_t* sums, int64_t clen,
                Reduce what, uint32_t* out, uint32_t* max_out, const ArgMaxSide* argmax = nullptr)
{
    if (what == kMedian) return median_array(ctx, n, beg, end, data, sums, clen, out);     // max_out belongs to the sum alone: not looked at
    if (what == kArgMax) return argmax ? argmax_array(ctx, n, beg, end, data, clen, *argmax, out) : IM_E_ARG;      // these arrays have no sums
    const bool minimum = what == kMinimum;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t sb = up256(sizeof(int32_t) * (size_t)n);
    int rc = ensure_ws(ctx, 4 * sb);
    if (rc) return rc;
    int32_t* d_beg = (int32_t*)ctx->ws;
    int32_t* d_end = (int32_t*)((char*)ctx->ws + sb);
    uint32_t* d_out = (uint32_t*)((char*)ctx->ws + 2 * sb);
    uint32_t* d_max = max_out ? (uint32_t*)((char*)ctx->ws + 3 * sb) : nullptr;
    HIP_TRY(ctx, hipMemcpyAsync(d_beg, beg, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_end, end, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (minimum) HIP_TRY(ctx, im::launch_span_query(n, d_beg, d_end, data, sums, clen, d_out, ctx->stream));
    else HIP_TRY(ctx, im::launch_depth_query_tiled(n, d_beg, d_end, data, sums, clen, d_out, d_max, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (max_out) HIP_TRY(ctx, hipMemcpyAsync(max_out, d_max, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return IM_OK;
}

// im_depth_query_max / im_depth_median / im_span_query / im_pairspan_query / im_clip_query
int query_contig_array(im_ctx* ctx, ContigArray im_ctx::*which, const char* family, int32_t n, const int32_t* beg, const int32_t* end, Reduce what,
                       uint32_t* out, const ArgMaxSide* argmax = nullptr, uint32_t* max_out = nullptr)
{
    if (!ctx || n < 0) return IM_E_ARG;
    const ContigArray& a = ctx->*which;
    if (a.len < 0) { set_err(ctx, "%s_build has not been called", family); return IM_E_ARG; }
    if (n == 0) return IM_OK;
    if (!beg || !end || !out) return IM_E_ARG;
    return query_array(ctx, n, beg, end, a.data, a.sums, a.len, what, out, max_out, argmax);
}

// im_depth_enable / im_span_enable / im_pairspan_enable / im_clip_enable: a genome-wide array and its sums, zeroed.  Each contig has its own
// run of sums (scans of different contigs may be in flight on different streams), at the same place in every array.  knob: what the family
// calls its flank in the messages; scanned = false: an array of point counts, which has no sums
int enable_genome_array(im_ctx* ctx, GenomeArray im_ctx::*which, const char* family, const int32_t* flank, int32_t min_mapq,
                        const char* knob = "flank", bool scanned = true)
{
    if (!ctx) return IM_E_ARG;
    if (!ctx->ref_ascii) { set_err(ctx, "im_set_reference has not been called"); return IM_E_ARG; }
    if (flank && *flank < 1) { set_err(ctx, "%s_enable: %s %d, must be >= 1", family, knob, *flank); return IM_E_ARG; }
    GenomeArray& g = ctx->*which;
    if (g.data) {
        if (flank && (*flank != g.flank || min_mapq != g.min_mapq)) { set_err(ctx, "%s_enable: already enabled with %s %d, min_mapq %d", family, knob, g.flank, g.min_mapq); return IM_E_ARG; }
        return IM_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int64_t ints = 0;
    std::vector<int64_t> sums_off;
    for (int32_t l : ctx->h_len) { sums_off.push_back(ints); ints += im::depth_sums_ints(l); }
    ctx->h_sums_off = sums_off;
    HIP_TRY(ctx, hipMalloc((void**)&g.data, (size_t)ctx->ref_total * sizeof(int32_t)));
    if (scanned) HIP_TRY(ctx, hipMalloc((void**)&g.sums, (size_t)(ints + 1) * sizeof(int32_t)));
    HIP_TRY(ctx, hipMemsetAsync(g.data, 0, (size_t)ctx->ref_total * sizeof(int32_t), ctx->stream));
    if (scanned) HIP_TRY(ctx, hipMemsetAsync(g.sums, 0, (size_t)(ints + 1) * sizeof(int32_t), ctx->stream));      // the arrival counters start at zero
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flank) { g.flank = *flank; g.min_mapq = min_mapq; }
    return IM_OK;
}

// im_depth_scan / im_span_scan / im_pairspan_scan: one launch, tile-local sums + exclusive tile offsets (the queries add them)
int scan_genome_array(im_ctx* ctx, GenomeArray im_ctx::*which, int32_t tid, void* stream)
{
    if (!ctx || !(ctx->*which).data || tid < 0 || tid >= ctx->n_contigs) return IM_E_ARG;
    const GenomeArray& g = ctx->*which;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_depth_scan_tiled(g.data + ctx->h_asc_off[tid], (int64_t)ctx->h_len[tid] + 1, g.sums + ctx->h_sums_off[tid], (hipStream_t)stream));
    return IM_OK;
}

// im_depth_reset / im_span_reset / im_pairspan_reset / im_clip_reset (both arrays)
int reset_genome_array(im_ctx* ctx, GenomeArray im_ctx::*which, int32_t tid, void* stream)
{
    if (!ctx || !(ctx->*which).data || tid < 0 || tid >= ctx->n_contigs) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_fill_zero((ctx->*which).data + ctx->h_asc_off[tid], (int64_t)ctx->h_len[tid] + 1, (hipStream_t)stream));
    return IM_OK;
}

// im_depth_query_max_tid / im_depth_median_tid / im_span_query_tid / im_pairspan_query_tid / im_clip_query_tid
int query_genome_array(im_ctx* ctx, GenomeArray im_ctx::*which, int32_t tid, int32_t n, const int32_t* beg, const int32_t* end, Reduce what,
                       uint32_t* out, uint32_t* max_out, const ArgMaxSide* argmax = nullptr)
{
    if (!ctx || n < 0 || !(ctx->*which).data || tid < 0 || tid >= ctx->n_contigs) return IM_E_ARG;
    if (n == 0) return IM_OK;
    if (!beg || !end || !out) return IM_E_ARG;
    const GenomeArray& g = ctx->*which;
    const int32_t* sums = g.sums ? g.sums + ctx->h_sums_off[tid] : nullptr;
    return query_array(ctx, n, beg, end, g.data + ctx->h_asc_off[tid], sums, ctx->h_len[tid], what, out, max_out, argmax);
}

im::RefDev ref_dev(const im_ctx* ctx)
{
    im::RefDev ref;
    ref.ascii = ctx->ref_ascii; ref.pk = reinterpret_cast<const uint8_t*>(ctx->ref_pk);
    ref.asc_off = ctx->d_asc_off; ref.pk_off = ctx->d_pk_off; ref.len = ctx->d_len; ref.n_contigs = ctx->n_contigs;
    return ref;
}

// A scatter call: the table of *which filled from the records by launch(reference, member, records, stream), nothing waited for
template <class Launch>
int keyed_scatter(im_ctx* ctx, KeyedMember im_ctx::*which, const im_dev_records* recs, void* stream, Launch launch)
{
    if (!ctx || !recs) return IM_E_ARG;
    const int rc = keyed_ready(ctx, ctx->*which, nullptr);
    if (rc) return rc;
    if (recs->n < 0) { set_err(ctx, "negative record count"); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, launch(ref_dev(ctx), ctx->*which, *recs, (hipStream_t)stream));
    return IM_OK;
}

// both link scatters take (reference, min_mapq, records, table, stream)
int link_scatter(im_ctx* ctx, KeyedMember im_ctx::*which, const im_dev_records* recs, void* stream, decltype(&im::launch_pairlink_scatter) launch)
{
    return keyed_scatter(ctx, which, recs, stream, [launch](const im::RefDev& ref, const KeyedMember& T, const im_dev_records& r, hipStream_t st) {
        return launch(ref, T.min_mapq, r, T, st); });
}

// The names as the blob contig_of_name (im_links.hip) reads: [bins][n][bin_start bins + 1][tid n][name_off n][name_len n][names], the
// entries in bin order; the bin of a name is its 32-bit FNV-1a hash & (bins - 1)
std::vector<uint8_t> split_name_blob(const std::vector<std::string>& names)
{
    const int32_t n = (int32_t)names.size();
    int32_t bins = 16;
    while (bins < n && bins < (1 << 20)) bins <<= 1;
    std::vector<uint32_t> bin(n);
    std::vector<int32_t> start(bins + 1, 0);
    for (int32_t i = 0; i < n; i++) {
        uint32_t h = 2166136261u;
        for (unsigned char c : names[i]) h = (h ^ c) * 16777619u;
        bin[i] = h & (uint32_t)(bins - 1);
        start[bin[i] + 1]++;
    }
    for (int32_t b = 0; b < bins; b++) start[b + 1] += start[b];
    std::vector<int32_t> at(start.begin(), start.end() - 1), e_tid(n), e_off(n), e_len(n);
    std::string bytes;
    for (int32_t i = 0; i < n; i++) {
        const int32_t e = at[bin[i]]++;
        e_tid[e] = i; e_off[e] = (int32_t)bytes.size(); e_len[e] = (int32_t)names[i].size();
        bytes += names[i];
    }
    std::vector<int32_t> words = {bins, n};
    words.insert(words.end(), start.begin(), start.end());
    words.insert(words.end(), e_tid.begin(), e_tid.end());
    words.insert(words.end(), e_off.begin(), e_off.end());
    words.insert(words.end(), e_len.begin(), e_len.end());
    std::vector<uint8_t> blob(words.size() * 4 + bytes.size());
    memcpy(blob.data(), words.data(), words.size() * 4);
    memcpy(blob.data() + words.size() * 4, bytes.data(), bytes.size());
    return blob;
}

// the sides of the add and the count calls (what: "link", "query")
int split_sides(im_ctx* ctx, const char* who, const char* what, int32_t n, const uint8_t* side1, const uint8_t* side2)
{
    for (int32_t i = 0; i < n; i++)
        if (side1[i] > 1 || side2[i] > 1) { set_err(ctx, "%s: %s %d: sides %d and %d, must be 0 (right) or 1 (left)", who, what, i, (int)side1[i], (int)side2[i]); return IM_E_ARG; }
    return IM_OK;
}

}  // namespace

extern "C" {

int im_abi_version(void) { return IM_ABI_VERSION; }

const char* im_last_error(const im_ctx* ctx) { return ctx ? ctx->err : g_err; }

int im_ctx_create(int device, im_ctx** out)
{
    if (!out) { set_err(nullptr, "out is NULL"); return IM_E_ARG; }
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_err(nullptr, "no HIP device available (%s); this library has no CPU path", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return IM_E_NOGPU;
    }
    if (device < 0 || device >= count) { set_err(nullptr, "device %d out of range (0..%d)", device, count - 1); return IM_E_ARG; }
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) { set_err(nullptr, "hipGetDeviceProperties: %s", hipGetErrorString(e)); return IM_E_HIP; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(nullptr, "device %d is %s; the kernels are built for gfx950 only", device, prop.gcnArchName);
        return IM_E_NOGPU;
    }
    im_ctx* ctx = new im_ctx();
    ctx->device = device;
    ctx->n_cu = prop.multiProcessorCount;
    e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { set_err(nullptr, "stream create: %s", hipGetErrorString(e)); delete ctx; return IM_E_HIP; }
    *out = ctx;
    return IM_OK;
}

void im_ctx_destroy(im_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    free_reference(ctx);
    if (ctx->ws) (void)hipFree(ctx->ws);
    if (ctx->med_scratch) (void)hipFree(ctx->med_scratch);
    free_array(ctx->depth);
    free_array(ctx->span);
    free_array(ctx->pair);
    free_array(ctx->clip_r);
    free_array(ctx->clip_l);
    if (ctx->rg_blob) (void)hipFree(ctx->rg_blob);
    if (ctx->any_list) (void)hipFree(ctx->any_list);
    if (ctx->any_counters) (void)hipFree(ctx->any_counters);
    if (ctx->any_arena) (void)hipFree(ctx->any_arena);
    if (ctx->pin) (void)hipHostFree(ctx->pin);
    for (int i = 0; i < 2; i++) {
        if (ctx->ev_in[i]) (void)hipEventDestroy(ctx->ev_in[i]);
        if (ctx->ev_k[i]) (void)hipEventDestroy(ctx->ev_k[i]);
        if (ctx->ev_out[i]) (void)hipEventDestroy(ctx->ev_out[i]);
    }
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->back_stream) (void)hipStreamDestroy(ctx->back_stream);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int im_set_reference(im_ctx* ctx, int32_t n_contigs, const char* const* seqs, const int64_t* lens)
{
    if (!ctx) return IM_E_ARG;
    if (n_contigs <= 0 || !seqs || !lens) { set_err(ctx, "bad reference arguments"); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    free_reference(ctx);
    // layout: [256 B zero pad][contig 0][>= 64 B zero pad, next start 256-aligned][contig 1]...
    std::vector<int64_t> asc_off(n_contigs), pk_off(n_contigs);
    std::vector<int32_t> len32(n_contigs);
    int64_t pos = 256;
    for (int32_t i = 0; i < n_contigs; i++) {
        if (lens[i] < 0 || lens[i] > 0x7fffff00LL) { set_err(ctx, "contig %d length %lld unsupported", i, (long long)lens[i]); return IM_E_ARG; }
        asc_off[i] = pos;
        pk_off[i] = pos / 4;
        len32[i] = (int32_t)lens[i];
        pos = (int64_t)up256((size_t)(pos + lens[i] + 64));
    }
    const int64_t total = pos + 256;                 // multiple of 256, hence of 32
    HIP_TRY(ctx, hipMalloc((void**)&ctx->ref_ascii, (size_t)total));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->ref_pk, (size_t)(total / 4 + 1024)));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_asc_off, sizeof(int64_t) * n_contigs));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_pk_off, sizeof(int64_t) * n_contigs));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_len, sizeof(int32_t) * n_contigs));
    HIP_TRY(ctx, hipMemsetAsync(ctx->ref_ascii, 0, (size_t)total, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->ref_pk, 0, (size_t)(total / 4 + 1024), ctx->stream));
    for (int32_t i = 0; i < n_contigs; i++)
        if (lens[i] > 0)
            HIP_TRY(ctx, hipMemcpyAsync(ctx->ref_ascii + asc_off[i], seqs[i], (size_t)lens[i], hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_asc_off, asc_off.data(), sizeof(int64_t) * n_contigs, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_pk_off, pk_off.data(), sizeof(int64_t) * n_contigs, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_len, len32.data(), sizeof(int32_t) * n_contigs, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, im::launch_pack_reference(ctx->ref_ascii, ctx->ref_pk, total, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->n_contigs = n_contigs;
    ctx->h_asc_off = asc_off; ctx->h_len = len32; ctx->ref_total = total;
    return IM_OK;
}

static int dev_realign(im_ctx* ctx, const im_params* params, const im_dev_batch* batch, int keep, const int32_t* n_dev, void* stream);

// The general pass: list what is left, size the arena from the longest read and the widest window on the list, work the list off.
// The list's size comes back to the host in between (a stream synchronisation: this pass is for inputs outside what sequencers
// deliver, and cannot be captured into a launch graph); one call at a time per context.
static int realign_any(im_ctx* ctx, const im::RealignArgs& a, int all, hipStream_t stream)
{
    if (a.batch.n <= 0) return IM_OK;
    std::lock_guard<std::mutex> lk(ctx->any_mu);
    if (!ctx->any_counters) HIP_TRY(ctx, hipMalloc((void**)&ctx->any_counters, 4 * sizeof(int32_t)));
    if (a.batch.n > ctx->any_list_cap) {
        if (ctx->any_list) { HIP_TRY(ctx, hipFree(ctx->any_list)); ctx->any_list = nullptr; ctx->any_list_cap = 0; }
        const int32_t cap = a.batch.n < (1 << 16) ? (1 << 16) : a.batch.n;
        HIP_TRY(ctx, hipMalloc((void**)&ctx->any_list, sizeof(int32_t) * (size_t)cap));
        ctx->any_list_cap = cap;
    }
    HIP_TRY(ctx, im::launch_realign_any_pick(a, all, ctx->any_list, ctx->any_counters, stream));
    int32_t h[4] = {0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(h, ctx->any_counters, sizeof h, hipMemcpyDeviceToHost, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    if (h[0] <= 0) return IM_OK;
    const int32_t max_read = h[1], max_window = h[2];
    // A batch of long reads is small against the chip (13 918 candidates of a 2 x 300 library are 218 waves of 64: less than one per CU
    // with three of its SIMDs idle): a wave then holds FEWER reads -- R = 8 .. 64 lanes with a read each, the others only help in the band
    // searches -- until every SIMD has a wave (a wave's instructions cost the same whatever the number of lanes at work: more waves than
    // SIMDs only add work -- 8 reads per wave took a 2 x 300 batch at -g 61 from 64 to 105 ms).
    const int64_t most = (int64_t)ctx->n_cu * 8, simds = (int64_t)ctx->n_cu * 4;
    int32_t lane_shift = 6;
    // (bands beyond the cooperative form's 32 diagonals: every lane on its own with a read each, as measured best)
    while (a.P.numgaps < 32u && lane_shift > 3 && ((int64_t)h[0] + (1 << (lane_shift - 1)) - 1) >> (lane_shift - 1) <= simds) lane_shift--;
    const size_t budget = (size_t)6 << 30;
    size_t per_wave = im::realign_any_arena_bytes(max_read, max_window, a.P.numgaps, lane_shift, 1);
    int64_t waves = ((int64_t)h[0] + (1 << lane_shift) - 1) >> lane_shift;
    if (waves > most) waves = most;
    if (per_wave * (size_t)waves > budget) waves = (int64_t)(budget / per_wave);
    if (waves < 1) waves = 1;
    const size_t need = per_wave * (size_t)waves;
    if (need > ctx->any_arena_bytes) {
        if (ctx->any_arena) { HIP_TRY(ctx, hipFree(ctx->any_arena)); ctx->any_arena = nullptr; ctx->any_arena_bytes = 0; }
        HIP_TRY(ctx, hipMalloc((void**)&ctx->any_arena, need));
        ctx->any_arena_bytes = need;
    }
    HIP_TRY(ctx, im::launch_realign_any(a, ctx->any_list, ctx->any_counters, ctx->any_arena, max_read, max_window, lane_shift, (int32_t)waves, stream));
    HIP_TRY(ctx, hipStreamSynchronize(stream));                                   // the list and the arena are free for the next call
    return IM_OK;
}

int im_dev_realign(im_ctx* ctx, const im_params* params, const im_dev_batch* batch, void* stream)
{
    return dev_realign(ctx, params, batch, 0, nullptr, stream);
}
int im_dev_realign_n(im_ctx* ctx, const im_params* params, const im_dev_batch* batch, const int32_t* n_dev, int32_t keep_slots, void* stream)
{
    return dev_realign(ctx, params, batch, keep_slots ? 1 : 0, n_dev, stream);
}
int im_dev_realign_keep(im_ctx* ctx, const im_params* params, const im_dev_batch* batch, void* stream)
{
    return dev_realign(ctx, params, batch, 1, nullptr, stream);
}

static int dev_realign(im_ctx* ctx, const im_params* params, const im_dev_batch* batch, int keep, const int32_t* n_dev, void* stream)
{
    if (!ctx || !batch) return IM_E_ARG;
    int rc = check_params(ctx, params);
    if (rc) return rc;
    if (!ctx->ref_ascii) { set_err(ctx, "im_set_reference has not been called"); return IM_E_ARG; }
    if (batch->n < 0) { set_err(ctx, "negative batch size"); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    im::RealignArgs a;
    a.ref = ref_dev(ctx);
    a.batch = *batch;
    a.P = *params;
    a.keep_slots = keep;
    a.n_dev = n_dev;
    a.first = 0;
    // Reads of up to 255 bases (1020 at numgaps == 0) and bands of up to 61 diagonals run in the kernels laid out for them; what
    // those leave IM_ST_UNSUPPORTED -- and every read when the band is wider than a wave -- takes the general pass behind them.
    const int expect = ctx->expect_len.load(std::memory_order_relaxed);
    const bool wide = params->numgaps > (uint32_t)im::kMaxWaveGaps;
    if (!wide) HIP_TRY(ctx, im::launch_realign(a, ctx->n_cu, (hipStream_t)stream));
    if (expect > im::kShortRead && params->numgaps == 0)
        HIP_TRY(ctx, im::launch_realign_long(a, ctx->n_cu, (hipStream_t)stream));
    if (wide || expect > IM_MAX_READ || (params->numgaps > 0 && expect > im::kShortRead))
        return realign_any(ctx, a, wide ? 1 : 0, (hipStream_t)stream);
    return IM_OK;
}

int im_dev_compact_results(im_ctx* ctx, const im_read_result* res, int32_t n, const int32_t* n_dev,
                           int32_t* status, int32_t* slot, im_read_result* compact, int32_t* count, void* stream)
{
    if (!ctx || n < 0 || !count || (n > 0 && (!res || !status || !slot || !compact))) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_compact_results(res, n, n_dev, status, slot, compact, count, ctx->n_cu, (hipStream_t)stream));
    return IM_OK;
}

int im_expect_read_length(im_ctx* ctx, int32_t max_len)
{
    if (!ctx) return IM_E_ARG;
    int cur = ctx->expect_len.load(std::memory_order_relaxed);
    while (max_len > cur && !ctx->expect_len.compare_exchange_weak(cur, max_len)) {}
    return IM_OK;
}

// ---- seam 0: record triage ---------------------------------------------------------------

int im_set_insert_ranges(im_ctx* ctx, int32_t n, const char* const* names_in, const int32_t* range_max)
{
    if (!ctx || n < 0 || (n > 0 && (!names_in || !range_max))) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // add_hashtable prepends to the chain of bin hash & 15 (src/hashtable.c:44-45): the chain order is the
    // REVERSE of the order of insertion
    std::vector<int32_t> bin(n);
    for (int32_t i = 0; i < n; i++) {
        const char* nm = names_in[i];
        const int len = (int)strlen(nm);
        uint32_t h = 5381u;
        for (int k = len - 1; k >= 0; k--) h += (h << 5) + (uint32_t)(int)nm[k];
        bin[i] = (int32_t)(h & 15u);
    }
    const int32_t m = n > 0 ? n : 1;
    std::vector<int32_t> bin_start(20, 0), name_off(m, 0), name_len(m, 0), rmax(m, 0);
    std::vector<uint8_t> names;
    int32_t e = 0;
    for (int b = 0; b < 16; b++) {
        bin_start[b] = e;
        for (int32_t i = n - 1; i >= 0; i--) {
            if (bin[i] != b) continue;
            name_off[e] = (int32_t)names.size();
            name_len[e] = (int32_t)strlen(names_in[i]);
            rmax[e] = range_max[i];
            names.insert(names.end(), names_in[i], names_in[i] + name_len[e] + 1);
            e++;
        }
    }
    bin_start[16] = e;
    std::vector<uint8_t> host((size_t)4 * (20 + 3 * (size_t)m) + names.size() + 8, 0);
    memcpy(host.data(), bin_start.data(), 80);
    memcpy(host.data() + 80, name_off.data(), 4 * (size_t)m);
    memcpy(host.data() + 80 + 4 * (size_t)m, name_len.data(), 4 * (size_t)m);
    memcpy(host.data() + 80 + 8 * (size_t)m, rmax.data(), 4 * (size_t)m);
    if (!names.empty()) memcpy(host.data() + 80 + 12 * (size_t)m, names.data(), names.size());
    const size_t total = (host.size() + 3) / 4 * 4;
    host.resize(total, 0);
    if (ctx->rg_blob) { HIP_TRY(ctx, hipFree(ctx->rg_blob)); ctx->rg_blob = nullptr; }
    HIP_TRY(ctx, hipMalloc(&ctx->rg_blob, total + 256));
    HIP_TRY(ctx, hipMemcpy(ctx->rg_blob, host.data(), total, hipMemcpyHostToDevice));
    ctx->rg.blob = (const uint8_t*)ctx->rg_blob; ctx->rg.n = n; ctx->rg.bytes = (int32_t)total;
    // "generic" as rg_lookup (im_rg.hpp) finds it: its bin's chain head to tail, strncmp over the seven bytes, the LAST hit wins
    {
        const char* gname = "generic";
        uint32_t h = 5381u;
        for (int k = 6; k >= 0; k--) h += (h << 5) + (uint32_t)(int)gname[k];
        const int gb = (int)(h & 15u);
        ctx->rg.generic_ok = 0; ctx->rg.generic_range = 0;
        for (int32_t k = bin_start[gb]; k < bin_start[gb + 1]; k++)
            if (name_len[k] >= 7 && memcmp(names.data() + name_off[k], gname, 7) == 0) { ctx->rg.generic_ok = 1; ctx->rg.generic_range = rmax[k]; }
    }
    return IM_OK;
}

size_t im_dev_triage_scratch_bytes(int32_t n_records) { return im::triage_scratch_bytes(n_records); }

int im_dev_triage_scratch_init(im_ctx* ctx, int32_t n_records, void* scratch, size_t scratch_bytes, void* stream)
{
    if (!ctx || !scratch || scratch_bytes < im::triage_scratch_bytes(n_records)) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t zb = 0;
    const size_t off = im::triage_scratch_zero_offset(n_records, &zb);
    HIP_TRY(ctx, hipMemsetAsync((char*)scratch + off, 0, zb, (hipStream_t)stream));
    return IM_OK;
}

int im_dev_triage(im_ctx* ctx, const im_triage_params* tp, const im_dev_records* recs, const im_dev_cands* out,
                  void* scratch, size_t scratch_bytes, void* stream)
{
    if (!ctx || !tp || !recs || !out) return IM_E_ARG;
    if (!ctx->ref_ascii) { set_err(ctx, "im_set_reference has not been called"); return IM_E_ARG; }
    if (!ctx->rg_blob) { set_err(ctx, "im_set_insert_ranges has not been called"); return IM_E_ARG; }
    if (recs->n < 0 || !out->counters || !out->cand_rec) { set_err(ctx, "bad triage arguments"); return IM_E_ARG; }
    if (scratch_bytes < im::triage_scratch_bytes(recs->n)) { set_err(ctx, "triage scratch too small"); return IM_E_ARG; }
    if (tp->want_depth && !ctx->all_depth.data) { set_err(ctx, "want_depth without im_depth_enable"); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_triage(ref_dev(ctx), ctx->rg, ctx->all_depth.data, *tp, *recs, *out, scratch, (hipStream_t)stream));
    return IM_OK;
}

// ---- seam 2, streaming form ------------------------------------------------------------------

int im_dev_flush_cut(im_ctx* ctx, const int32_t* cls, const int32_t* b1, const int32_t* b2, int32_t* consumed,
                     int32_t a0, int32_t a1, int32_t b0, int32_t b1_end, int32_t marker, int32_t flush_id,
                     uint64_t* cut_word, void* stream)
{
    if (!ctx || !cut_word || flush_id <= 0) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_flush_cut(cls, b1, b2, consumed, a0, a1, b0, b1_end, marker, flush_id, cut_word, nullptr, nullptr, 0, (hipStream_t)stream));
    return IM_OK;
}

int im_dev_flush_cut_rec(im_ctx* ctx, const int32_t* cls, const int32_t* b1, const int32_t* b2, int32_t* consumed,
                         int32_t rec0, int32_t rec1, const int32_t* cand_rec, const int32_t* n_cand_dev, int32_t cand_cap,
                         int32_t b0, int32_t b1_end, int32_t marker, int32_t flush_id, uint64_t* cut_word, void* stream)
{
    if (!ctx || !cut_word || flush_id <= 0 || !cand_rec || !n_cand_dev || cand_cap < 0) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_flush_cut(cls, b1, b2, consumed, rec0, rec1, b0, b1_end, marker, flush_id, cut_word, cand_rec, n_cand_dev, cand_cap, (hipStream_t)stream));
    return IM_OK;
}

int im_dev_flush_cuts(im_ctx* ctx, const im_flush_desc* desc_dev, int32_t n_flushes,
                      const int32_t* cls, const int32_t* b1, const int32_t* b2, int32_t* consumed,
                      const int32_t* cand_rec, const int32_t* n_cand_dev, int32_t cand_cap, int32_t pe_base, int32_t pe_count, void* stream)
{
    if (!ctx || n_flushes < 0 || !desc_dev || !cand_rec || !n_cand_dev || pe_count < 0) return IM_E_ARG;
    if ((((uintptr_t)cls) | ((uintptr_t)b1) | ((uintptr_t)b2) | ((uintptr_t)consumed)) & 15u) { set_err(ctx, "im_dev_flush_cuts: the slot arrays must be 16-byte aligned"); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_flush_seq(desc_dev, n_flushes, cls, b1, b2, consumed, cand_rec, n_cand_dev, cand_cap, pe_base, pe_count, (hipStream_t)stream));
    return IM_OK;
}

size_t im_dev_flushgroup_scratch_bytes(int32_t n_slots_cap, int32_t n_flushes_cap) { return im::flushgroup_scratch_bytes(n_slots_cap, n_flushes_cap); }

int im_dev_flushgroup_scratch_init(im_ctx* ctx, int32_t n_slots_cap, int32_t n_flushes_cap, void* scratch, size_t scratch_bytes, void* stream)
{
    if (!ctx || !scratch || n_slots_cap < 0 || n_flushes_cap < 0 || scratch_bytes < im::flushgroup_scratch_bytes(n_slots_cap, n_flushes_cap)) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_flushgroup_init(n_slots_cap, n_flushes_cap, scratch, (hipStream_t)stream));
    { std::lock_guard<std::mutex> lk(ctx->gb_mu); ctx->fg_layout[scratch] = std::make_pair(n_slots_cap, n_flushes_cap); }
    return IM_OK;
}

int im_dev_flush_groupby(im_ctx* ctx, const im_flush_desc* desc_dev, int32_t n_flushes,
                         const int32_t* cls, const int32_t* b1, const int32_t* b2, int32_t* consumed,
                         const int32_t* cand_rec, const int32_t* n_cand_dev, int32_t cand_cap, int32_t pe_base, int32_t pe_count, int32_t tie_desc,
                         int32_t* order, int32_t* cl_key, int32_t* cl_first, int32_t* cl_count, int32_t* counts,
                         void* scratch, size_t scratch_bytes, void* stream)
{
    if (!ctx || n_flushes < 0 || !desc_dev || !cand_rec || !n_cand_dev || cand_cap < 0 || pe_count < 0 || !counts || !scratch) return IM_E_ARG;
    if (((((uintptr_t)cls) | ((uintptr_t)b1) | ((uintptr_t)b2) | ((uintptr_t)consumed) | ((uintptr_t)desc_dev) | ((uintptr_t)cl_key)) & 15u) || (((uintptr_t)counts) & 7u)) {
        set_err(ctx, "im_dev_flush_groupby: the slot arrays, desc and cl_key must be 16-byte aligned, counts 8-byte aligned"); return IM_E_ARG;
    }
    std::pair<int32_t, int32_t> lay(-1, -1);
    {
        std::lock_guard<std::mutex> lk(ctx->gb_mu);
        auto it = ctx->fg_layout.find(scratch);
        if (it != ctx->fg_layout.end()) lay = it->second;
    }
    if (lay.first < 0) { set_err(ctx, "flush + group-by scratch was not initialised (im_dev_flushgroup_scratch_init)"); return IM_E_ARG; }
    if ((int64_t)cand_cap * IM_MAX_EV > lay.first || n_flushes > lay.second || scratch_bytes < im::flushgroup_scratch_bytes(lay.first, lay.second)) {
        set_err(ctx, "flush + group-by scratch too small"); return IM_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_flush_groupby(lay.first, lay.second, desc_dev, n_flushes, cls, b1, b2, consumed, cand_rec, n_cand_dev, cand_cap, pe_base, pe_count,
                                          tie_desc, order, cl_key, cl_first, cl_count, counts, scratch, (hipStream_t)stream));
    return IM_OK;
}

size_t im_dev_groupby_scratch_bytes(int32_t n_slots) { return im::groupby_scratch_bytes(n_slots); }

int im_dev_groupby_scratch_init(im_ctx* ctx, int32_t n_slots, void* scratch, size_t scratch_bytes, void* stream)
{
    if (!ctx || !scratch || scratch_bytes < im::groupby_scratch_bytes(n_slots)) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_groupby_init(n_slots, scratch, (hipStream_t)stream));
    { std::lock_guard<std::mutex> lk(ctx->gb_mu); ctx->gb_layout[scratch] = n_slots; }
    return IM_OK;
}

// the slot count a group-by scratch was initialised for, or -1
static int32_t groupby_layout(im_ctx* ctx, void* scratch)
{
    std::lock_guard<std::mutex> lk(ctx->gb_mu);
    auto it = ctx->gb_layout.find(scratch);
    return it == ctx->gb_layout.end() ? -1 : it->second;
}

int im_dev_cluster_groupby(im_ctx* ctx, int32_t n_slots, const int32_t* cls, const int32_t* b1, const int32_t* b2,
                           const int32_t* consumed, int32_t tie_desc,
                           int32_t* order, int32_t* cl_key, int32_t* cl_first, int32_t* cl_count, int32_t* counts,
                           void* scratch, size_t scratch_bytes, void* stream)
{
    if (!ctx || n_slots < 0 || !counts) return IM_E_ARG;
    const int32_t n_layout = groupby_layout(ctx, scratch);
    if (n_layout < 0) { set_err(ctx, "group-by scratch was not initialised (im_dev_groupby_scratch_init)"); return IM_E_ARG; }
    if (n_slots > n_layout || scratch_bytes < im::groupby_scratch_bytes(n_layout)) { set_err(ctx, "group-by scratch too small"); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_slots == 0) { HIP_TRY(ctx, hipMemsetAsync(counts, 0, 8, (hipStream_t)stream)); return IM_OK; }
    HIP_TRY(ctx, im::launch_groupby(n_layout, n_slots, nullptr, cls, b1, b2, consumed, tie_desc, order, cl_key, cl_first, cl_count, counts, scratch, (hipStream_t)stream));
    return IM_OK;
}

int im_dev_cluster_groupby_n(im_ctx* ctx, int32_t n_slots_cap, const int32_t* n_cand_dev, const int32_t* cls, const int32_t* b1, const int32_t* b2,
                             const int32_t* consumed, int32_t tie_desc,
                             int32_t* order, int32_t* cl_key, int32_t* cl_first, int32_t* cl_count, int32_t* counts,
                             void* scratch, size_t scratch_bytes, void* stream)
{
    if (!ctx || n_slots_cap <= 0 || !counts || !n_cand_dev) return IM_E_ARG;
    const int32_t n_layout = groupby_layout(ctx, scratch);
    if (n_layout < 0) { set_err(ctx, "group-by scratch was not initialised (im_dev_groupby_scratch_init)"); return IM_E_ARG; }
    if (n_slots_cap > n_layout || scratch_bytes < im::groupby_scratch_bytes(n_layout)) { set_err(ctx, "group-by scratch too small"); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_groupby(n_layout, n_slots_cap, n_cand_dev, cls, b1, b2, consumed, tie_desc, order, cl_key, cl_first, cl_count, counts, scratch, (hipStream_t)stream));
    return IM_OK;
}

// ---- seam 3, genome-wide form ------------------------------------------------------------------

int im_depth_enable(im_ctx* ctx) { return enable_genome_array(ctx, &im_ctx::all_depth, "im_depth", nullptr, 0); }
int im_depth_scan(im_ctx* ctx, int32_t tid, void* stream) { return scan_genome_array(ctx, &im_ctx::all_depth, tid, stream); }
int im_depth_reset(im_ctx* ctx, int32_t tid, void* stream) { return reset_genome_array(ctx, &im_ctx::all_depth, tid, stream); }

int im_depth_allreduce(im_ctx* ctx, im_comm* comm)
{
    if (!ctx || !comm) return IM_E_ARG;
    if (!ctx->all_depth.data) { set_err(ctx, "im_depth_enable has not been called"); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t total = (size_t)ctx->ref_total, step = (size_t)1 << 28;           // 1 GiB of int32 per call
    for (size_t at = 0; at < total; at += step) {
        const size_t n = total - at < step ? total - at : step;
        if (im_comm_allreduce_sum_i32(comm, ctx->all_depth.data + at, n, ctx->stream) != IM_OK) { set_err(ctx, "%s", im_comm_last_error()); return IM_E_HIP; }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return IM_OK;
}

int im_depth_query_max_tid(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* sum_out, uint32_t* max_out)
{ return query_genome_array(ctx, &im_ctx::all_depth, tid, n, beg, end, kSum, sum_out, max_out); }

int im_depth_query_tid(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* sum_out)
{ return im_depth_query_max_tid(ctx, tid, n, beg, end, sum_out, nullptr); }

int im_depth_median_tid(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* med_out)
{ return query_genome_array(ctx, &im_ctx::all_depth, tid, n, beg, end, kMedian, med_out, nullptr); }

// Host-buffer entry point.  The batch is cut into chunks that travel through a two-slot pipeline: chunk c is
// packed into PINNED staging memory and copied in on one copy stream while chunk c-1 runs on the compute stream
// and the results of chunk c-2 come back on another (hipMemcpyAsync from / to pinned memory throughout, stream-to-stream
// events between the three stages), so that PCIe, the kernel and the host-side packing overlap.
int im_realign_batch(im_ctx* ctx, const im_params* params, const im_read_batch* batch, im_read_result* out)
{
    if (!ctx || !batch || !out) return IM_E_ARG;
    int rc = check_params(ctx, params);
    if (rc) return rc;
    const int32_t n = batch->n;
    if (n < 0) { set_err(ctx, "negative batch size"); return IM_E_ARG; }
    if (n == 0) return IM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->copy_stream) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->back_stream, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_in[i], hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_k[i], hipEventDisableTiming));
            HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_out[i], hipEventDisableTiming));
        }
    }
    for (int32_t i = 0; i < n; i++) {
        const int64_t l = batch->base_off[i + 1] - batch->base_off[i];
        if (l < 0 || l > 0x7fffffff) { set_err(ctx, "read %d has a bad length", i); return IM_E_ARG; }
    }

    constexpr int32_t kChunk = 32768;                      // reads per pipeline stage
    const int32_t cn = n < kChunk ? n : kChunk;
    // per-slot layout (identical on the device and in pinned memory): bases (worst case from the batch), off, len, tid, anchor, range, results
    int64_t max_bases = 0;
    for (int32_t c0 = 0; c0 < n; c0 += kChunk) {
        const int32_t c1 = c0 + kChunk < n ? c0 + kChunk : n;
        int64_t b = 0;
        for (int32_t i = c0; i < c1; i++) b += ((batch->base_off[i + 1] - batch->base_off[i]) + 3) & ~(int64_t)3;
        if (b > max_bases) max_bases = b;
    }
    const size_t bases_bytes = up256((size_t)max_bases + 16);
    const size_t off_bytes = up256(sizeof(int64_t) * (size_t)cn);
    const size_t i32_bytes = up256(sizeof(int32_t) * (size_t)cn);
    const size_t res_bytes = up256(sizeof(im_read_result) * (size_t)cn);
    const size_t in_bytes = bases_bytes + off_bytes + 4 * i32_bytes;
    const size_t slot_bytes = in_bytes + res_bytes;
    rc = ensure_ws(ctx, 2 * slot_bytes);
    if (rc) return rc;
    rc = ensure_pin(ctx, 2 * slot_bytes);
    if (rc) return rc;

    const int32_t nchunks = (n + kChunk - 1) / kChunk;
    auto collect = [&](int32_t c) -> int {                 // results of chunk c: pinned -> caller
        const int sl = c & 1;
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev_out[sl]));
        const int32_t c0 = c * kChunk, c1 = c0 + kChunk < n ? c0 + kChunk : n;
        memcpy(out + c0, (char*)ctx->pin + (size_t)sl * slot_bytes + in_bytes, sizeof(im_read_result) * (size_t)(c1 - c0));
        return IM_OK;
    };
    for (int32_t c = 0; c < nchunks; c++) {
        const int sl = c & 1;
        if (c >= 2) { rc = collect(c - 2); if (rc) return rc; }      // frees this slot's pinned and device halves
        const int32_t c0 = c * kChunk, c1 = c0 + kChunk < n ? c0 + kChunk : n, m = c1 - c0;
        char* hp = (char*)ctx->pin + (size_t)sl * slot_bytes;
        char* dp = (char*)ctx->ws + (size_t)sl * slot_bytes;
        uint8_t* h_bases = (uint8_t*)hp;
        int64_t* h_off = (int64_t*)(hp + bases_bytes);
        int32_t* h_len = (int32_t*)(hp + bases_bytes + off_bytes);
        int32_t* h_tid = (int32_t*)(hp + bases_bytes + off_bytes + i32_bytes);
        int32_t* h_anchor = (int32_t*)(hp + bases_bytes + off_bytes + 2 * i32_bytes);
        int32_t* h_range = (int32_t*)(hp + bases_bytes + off_bytes + 3 * i32_bytes);
        // re-pack the reads at 4-byte aligned offsets (device layout requirement), straight into pinned memory
        int64_t pos = 0, longest = 0;
        for (int32_t i = 0; i < m; i++) {
            const int64_t l = batch->base_off[c0 + i + 1] - batch->base_off[c0 + i];
            h_off[i] = pos; h_len[i] = (int32_t)l;
            if (l > longest) longest = l;
            memcpy(h_bases + pos, batch->bases + batch->base_off[c0 + i], (size_t)l);
            const int64_t padded = (l + 3) & ~(int64_t)3;
            memset(h_bases + pos + l, 0, (size_t)(padded - l));
            pos += padded;
        }
        memset(h_bases + pos, 0, 16);
        memcpy(h_tid, batch->tid + c0, sizeof(int32_t) * (size_t)m);
        memcpy(h_anchor, batch->anchor + c0, sizeof(int32_t) * (size_t)m);
        memcpy(h_range, batch->range_max + c0, sizeof(int32_t) * (size_t)m);
        if (longest > im::kShortRead) im_expect_read_length(ctx, (int32_t)longest);
        HIP_TRY(ctx, hipMemcpyAsync(dp, hp, in_bytes, hipMemcpyHostToDevice, ctx->copy_stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_in[sl], ctx->copy_stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_in[sl], 0));

        im_dev_batch db;
        db.n = m; db.bases = (uint8_t*)dp; db.base_off = (int64_t*)(dp + bases_bytes);
        db.read_len = (int32_t*)(dp + bases_bytes + off_bytes); db.tid = (int32_t*)(dp + bases_bytes + off_bytes + i32_bytes);
        db.anchor = (int32_t*)(dp + bases_bytes + off_bytes + 2 * i32_bytes); db.range_max = (int32_t*)(dp + bases_bytes + off_bytes + 3 * i32_bytes);
        db.out = (im_read_result*)(dp + in_bytes);
        db.ev_cls = nullptr; db.ev_b1 = nullptr; db.ev_b2 = nullptr;
        rc = im_dev_realign(ctx, params, &db, ctx->stream);
        if (rc) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->ev_k[sl], ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->back_stream, ctx->ev_k[sl], 0));
        HIP_TRY(ctx, hipMemcpyAsync(hp + in_bytes, dp + in_bytes, sizeof(im_read_result) * (size_t)m, hipMemcpyDeviceToHost, ctx->back_stream));
        HIP_TRY(ctx, hipEventRecord(ctx->ev_out[sl], ctx->back_stream));
    }
    for (int32_t c = nchunks >= 2 ? nchunks - 2 : 0; c < nchunks; c++) { rc = collect(c); if (rc) return rc; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

    int worst = IM_OK;
    for (int32_t i = 0; i < n; i++) {
        const int st = out[i].status;
        if (st == IM_ST_ABORT && worst == IM_OK) { worst = IM_E_ABORT; set_err(ctx, "read %d: the reference would abort on this input", i); }
        else if (st == IM_ST_OVERFLOW && worst == IM_OK) { worst = IM_E_OVERFLOW; set_err(ctx, "read %d: more than IM_MAX_OPS segments or IM_MAX_EV indels", i); }
        else if (st == IM_ST_UNSUPPORTED && worst == IM_OK) { worst = IM_E_UNSUPPORTED; set_err(ctx, "read %d: longer than IM_MAX_READ=%d%s", i, IM_MAX_READ, params->numgaps ? ", or than 255 with numgaps > 0" : ""); }
    }
    return worst;
}

int im_depth_build(im_ctx* ctx, int64_t contig_len, int32_t n_seg, const int32_t* seg_start, const int32_t* seg_len)
{ return build_array(ctx, &im_ctx::depth, "im_depth", contig_len, n_seg, seg_start, seg_len, nullptr); }

int im_depth_query_max(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* sum_out, uint32_t* max_out)
{ return query_contig_array(ctx, &im_ctx::depth, "im_depth", n, beg, end, kSum, sum_out, nullptr, max_out); }

int im_depth_query(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* sum_out)
{ return im_depth_query_max(ctx, n, beg, end, sum_out, nullptr); }

int im_depth_median(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* med_out)
{ return query_contig_array(ctx, &im_ctx::depth, "im_depth", n, beg, end, kMedian, med_out); }

// ---- reference-spanning read counts (the genotype columns) ------------------------------------

int im_span_enable(im_ctx* ctx, int32_t flank, int32_t min_mapq) { return enable_genome_array(ctx, &im_ctx::all_span, "im_span", &flank, min_mapq); }

int im_dev_span_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream)
{
    if (!ctx || !recs) return IM_E_ARG;
    const GenomeArray& g = ctx->all_span;
    if (!g.data) { set_err(ctx, "im_span_enable has not been called"); return IM_E_ARG; }
    if (recs->n < 0) { set_err(ctx, "negative record count"); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_span_scatter(ref_dev(ctx), g.flank, g.min_mapq, *recs, g.data, (hipStream_t)stream));
    return IM_OK;
}

int im_span_scan(im_ctx* ctx, int32_t tid, void* stream) { return scan_genome_array(ctx, &im_ctx::all_span, tid, stream); }
int im_span_reset(im_ctx* ctx, int32_t tid, void* stream) { return reset_genome_array(ctx, &im_ctx::all_span, tid, stream); }

int im_span_query_tid(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* min_out)
{ return query_genome_array(ctx, &im_ctx::all_span, tid, n, beg, end, kMinimum, min_out, nullptr); }

// A list of ends, each on its own contig: every range is checked here, before anything is copied.  [tid][pos][sums_off, 8 bytes] in, one
// launch, out back, one wait.  The kernel finds a contig's run of the array through the reference's device columns; where the contig
// keeps its tile offsets is known on the host alone (h_sums_off), so it travels as a column per end.
int im_span_query_ends(im_ctx* ctx, int32_t n, const int32_t* tid, const int32_t* pos, int32_t slack, uint32_t* min_out)
{
    if (!ctx) return IM_E_ARG;
    const char* who = "im_span_query_ends";
    const GenomeArray& g = ctx->all_span;
    if (!g.data) { set_err(ctx, "%s: im_span_enable has not been called", who); return IM_E_ARG; }
    if (n < 0) { set_err(ctx, "%s: n %d, must be >= 0", who, n); return IM_E_ARG; }
    if (slack < 0 || slack > 255) { set_err(ctx, "%s: slack %d, must be 0 .. 255", who, slack); return IM_E_ARG; }
    if (n == 0) return IM_OK;
    if (!tid || !pos || !min_out) { set_err(ctx, "%s: a null column with n %d", who, n); return IM_E_ARG; }
    std::vector<int64_t> sums_off((size_t)n);
    for (int32_t k = 0; k < n; k++) {
        if (tid[k] < 0 || tid[k] >= ctx->n_contigs) { set_err(ctx, "%s: end %d: tid %d, the reference has %d contigs", who, k, tid[k], ctx->n_contigs); return IM_E_ARG; }
        if (pos[k] < 0 || pos[k] > ctx->h_len[tid[k]]) { set_err(ctx, "%s: end %d: pos %d, must be 0 .. %d on contig %d", who, k, pos[k], ctx->h_len[tid[k]], tid[k]); return IM_E_ARG; }
        sums_off[k] = ctx->h_sums_off[tid[k]];
    }
    WsColumns C;
    int rc = ws_columns(ctx, n, 5, &C);
    if (rc || (rc = C.down(0, tid, 4)) || (rc = C.down(1, pos, 4)) || (rc = C.down(2, sums_off.data(), 8))) return rc;
    im::SpanEndsArgs A;
    A.n = n; A.slack = slack; A.tid = C.at<int32_t>(0); A.pos = C.at<int32_t>(1); A.sums_off = C.at<int64_t>(2);
    A.asc_off = ctx->d_asc_off; A.len = ctx->d_len; A.n_contigs = ctx->n_contigs; A.span = g.data; A.sums = g.sums; A.out = C.at<uint32_t>(4);
    HIP_TRY(ctx, im::launch_span_query_ends(A, ctx->stream));
    if ((rc = C.up(4, min_out, 4))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return IM_OK;
}

int im_span_build(im_ctx* ctx, int64_t contig_len, int32_t n_run, const int32_t* run_start, const int32_t* run_len, int32_t flank)
{ return build_array(ctx, &im_ctx::span, "im_span", contig_len, n_run, run_start, run_len, &flank); }

int im_span_query(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* min_out)
{ return query_contig_array(ctx, &im_ctx::span, "im_span", n, beg, end, kMinimum, min_out); }

// ---- concordant-pair counts (the genotype columns of PAIRED_READ records) ----------------------

int im_pairspan_enable(im_ctx* ctx, int32_t flank, int32_t min_mapq) { return enable_genome_array(ctx, &im_ctx::all_pair, "im_pairspan", &flank, min_mapq); }

int im_dev_pairspan_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream)
{
    if (!ctx || !recs) return IM_E_ARG;
    const GenomeArray& g = ctx->all_pair;
    if (!g.data) { set_err(ctx, "im_pairspan_enable has not been called"); return IM_E_ARG; }
    if (!ctx->rg_blob) { set_err(ctx, "im_set_insert_ranges has not been called"); return IM_E_ARG; }
    if (recs->n < 0) { set_err(ctx, "negative record count"); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_pair_scatter(ref_dev(ctx), ctx->rg, g.flank, g.min_mapq, *recs, g.data, (hipStream_t)stream));
    return IM_OK;
}

int im_pairspan_scan(im_ctx* ctx, int32_t tid, void* stream) { return scan_genome_array(ctx, &im_ctx::all_pair, tid, stream); }
int im_pairspan_reset(im_ctx* ctx, int32_t tid, void* stream) { return reset_genome_array(ctx, &im_ctx::all_pair, tid, stream); }

int im_pairspan_query_tid(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* min_out)
{ return query_genome_array(ctx, &im_ctx::all_pair, tid, n, beg, end, kMinimum, min_out, nullptr); }

int im_pairspan_build(im_ctx* ctx, int64_t contig_len, int32_t n_frag, const int32_t* frag_start, const int32_t* frag_len, int32_t flank)
{ return build_array(ctx, &im_ctx::pair, "im_pairspan", contig_len, n_frag, frag_start, frag_len, &flank); }

int im_pairspan_query(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* min_out)
{ return query_contig_array(ctx, &im_ctx::pair, "im_pairspan", n, beg, end, kMinimum, min_out); }

// ---- clipped-read counts (the breakpoint evidence of large deletions) --------------------------

int im_clip_enable(im_ctx* ctx, int32_t min_clip, int32_t min_mapq)
{
    const int rc = enable_genome_array(ctx, &im_ctx::all_clip_r, "im_clip", &min_clip, min_mapq, "min_clip", false);
    return rc ? rc : enable_genome_array(ctx, &im_ctx::all_clip_l, "im_clip", &min_clip, min_mapq, "min_clip", false);
}

int im_dev_clip_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream)
{
    if (!ctx || !recs) return IM_E_ARG;
    const GenomeArray& g = ctx->all_clip_r;
    if (!g.data || !ctx->all_clip_l.data) { set_err(ctx, "im_clip_enable has not been called"); return IM_E_ARG; }
    if (recs->n < 0) { set_err(ctx, "negative record count"); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, im::launch_clip_scatter(ref_dev(ctx), g.flank, g.min_mapq, *recs, g.data, ctx->all_clip_l.data, (hipStream_t)stream));
    return IM_OK;
}

int im_clip_reset(im_ctx* ctx, int32_t tid, void* stream)
{
    if (!ctx || !ctx->all_clip_l.data) return IM_E_ARG;
    const int rc = reset_genome_array(ctx, &im_ctx::all_clip_r, tid, stream);
    return rc ? rc : reset_genome_array(ctx, &im_ctx::all_clip_l, tid, stream);
}

int im_clip_query_tid(im_ctx* ctx, int32_t tid, int32_t n, const uint8_t* side, const int32_t* beg, const int32_t* end, uint32_t* count_out, int32_t* pos_out)
{
    if (!ctx || !ctx->all_clip_l.data || tid < 0 || tid >= ctx->n_contigs) return IM_E_ARG;
    const ArgMaxSide x = {side, ctx->all_clip_l.data + ctx->h_asc_off[tid], pos_out};
    return query_genome_array(ctx, &im_ctx::all_clip_r, tid, n, beg, end, kArgMax, count_out, nullptr, &x);
}

// the host names the events: both arrays grown through the family's helper, cleared, one count per event, wait
int im_clip_build(im_ctx* ctx, int64_t contig_len, int32_t n, const int32_t* pos, const uint8_t* side)
{
    if (!ctx || contig_len < 0 || contig_len > 0x7fffff00LL || n < 0 || (n > 0 && (!pos || !side))) return IM_E_ARG;
    for (int32_t i = 0; i < n; i++) if (side[i] > 1) { set_err(ctx, "im_clip_build: event %d: side %d, must be 0 (right) or 1 (left)", i, (int)side[i]); return IM_E_ARG; }
    int rc = grow_array(ctx, ctx->clip_r, contig_len, false);
    if (!rc) rc = grow_array(ctx, ctx->clip_l, contig_len, false);
    if (rc) return rc;
    const size_t sb = up256(sizeof(int32_t) * (size_t)(n ? n : 1));
    rc = ensure_ws(ctx, 2 * sb);
    if (rc) return rc;
    int32_t* d_pos = (int32_t*)ctx->ws;
    uint8_t* d_side = (uint8_t*)ctx->ws + sb;
    if (n > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(d_pos, pos, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_side, side, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, im::launch_clip_build(contig_len, n, d_pos, d_side, ctx->clip_r.data, ctx->clip_l.data, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->clip_r.len = ctx->clip_l.len = contig_len;
    return IM_OK;
}

int im_clip_query(im_ctx* ctx, int32_t n, const uint8_t* side, const int32_t* beg, const int32_t* end, uint32_t* count_out, int32_t* pos_out)
{
    if (!ctx) return IM_E_ARG;
    const ArgMaxSide x = {side, ctx->clip_l.data, pos_out};
    return query_contig_array(ctx, &im_ctx::clip_r, "im_clip", n, beg, end, kArgMax, count_out, &x);
}

// the two clip arrays a search reads, and their length
struct ClipArrays { const int32_t* right; const int32_t* left; int64_t clen; };

// the resident arrays of contig tid
static int resident_clip(im_ctx* ctx, int32_t tid, ClipArrays* A)
{
    if (!ctx || !ctx->all_clip_r.data || !ctx->all_clip_l.data || tid < 0 || tid >= ctx->n_contigs) return IM_E_ARG;
    const int64_t at = ctx->h_asc_off[tid];
    *A = {ctx->all_clip_r.data + at, ctx->all_clip_l.data + at, ctx->h_len[tid]};
    return IM_OK;
}

// the arrays of the last im_clip_build; tid: the contig they must be the arrays of (a search that reads the reference), or null
static int built_clip(im_ctx* ctx, const char* who, const int32_t* tid, ClipArrays* A)
{
    if (!ctx || (tid && (*tid < 0 || *tid >= ctx->n_contigs))) return IM_E_ARG;
    if (ctx->clip_r.len < 0 || ctx->clip_l.len < 0) { set_err(ctx, "im_clip_build has not been called"); return IM_E_ARG; }
    if (tid && ctx->clip_r.len != ctx->h_len[*tid]) { set_err(ctx, "%s: the arrays of the last im_clip_build are not contig %d's", who, *tid); return IM_E_ARG; }
    *A = {ctx->clip_r.data, ctx->clip_l.data, ctx->clip_r.len};
    return IM_OK;
}

// k device columns of n 32-bit words down, the rows sorted by up to three key columns (the first decides, then the next), into the
// host columns.  Key columns hold positions, counts or a side, never a negative value, so a row's keys and its index pack into two
// 64-bit words that sort as plain integers: a comparator that walks a list of columns cost a third more on a list of peaks.
static int sorted_columns(im_ctx* ctx, int k, void* const* d_col, uint32_t n, std::initializer_list<int> keys, void* const* out)
{
    if (n == 0) return IM_OK;
    std::vector<int32_t> h((size_t)k * n);
    for (int c = 0; c < k; c++) HIP_TRY(ctx, hipMemcpyAsync(h.data() + (size_t)c * n, d_col[c], sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<std::pair<uint64_t, uint64_t>> row(n);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t v[3] = {0, 0, 0};
        int j = 0;
        for (int c : keys) v[j++] = (uint32_t)h[(size_t)c * n + i];
        row[i] = {((uint64_t)v[0] << 32) | v[1], ((uint64_t)v[2] << 32) | i};
    }
    std::sort(row.begin(), row.end());
    for (int c = 0; c < k; c++) for (uint32_t i = 0; i < n; i++) ((int32_t*)out[c])[i] = h[(size_t)c * n + (uint32_t)row[i].second];
    return IM_OK;
}

// the facing piles of one contig's two arrays: the counter and four arrays of cap in the workspace, one launch, the counter back,
// then what was found (piles are few), sorted by pr here (a position is a pile once)
static int facing_arrays(im_ctx* ctx, const char* who, const ClipArrays& A, int32_t min_reads, int32_t max_overlap, int32_t cap, int32_t* pr, int32_t* pl,
                         uint32_t* cr, uint32_t* cl, int32_t* n_found)
{
    if (min_reads < 1) { set_err(ctx, "%s: min_reads %d, must be >= 1", who, min_reads); return IM_E_ARG; }
    if (max_overlap < 0 || max_overlap > 64) { set_err(ctx, "%s: max_overlap %d, must be 0 .. 64", who, max_overlap); return IM_E_ARG; }
    if (cap < 0) { set_err(ctx, "%s: cap %d, must be >= 0", who, cap); return IM_E_ARG; }
    if (!n_found || (cap > 0 && (!pr || !pl || !cr || !cl))) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t sb = up256(sizeof(int32_t) * (size_t)(cap ? cap : 1));
    int rc = ensure_ws(ctx, 256 + 4 * sb);
    if (rc) return rc;
    uint32_t* d_count = (uint32_t*)ctx->ws;
    void* d_out[4];
    for (int k = 0; k < 4; k++) d_out[k] = (char*)ctx->ws + 256 + k * sb;
    uint32_t found = 0;
    HIP_TRY(ctx, im::launch_clip_facing(A.right, A.left, A.clen, min_reads, max_overlap, cap, (int32_t*)d_out[0], (int32_t*)d_out[1], (uint32_t*)d_out[2],
                                        (uint32_t*)d_out[3], d_count, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&found, d_count, sizeof found, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_found = (int32_t)found;
    if (found > (uint32_t)cap) return IM_OK;                        // more than cap: the caller asks again
    void* const out[4] = {pr, pl, cr, cl};
    return sorted_columns(ctx, 4, d_out, found, {0}, out);
}

int im_clip_facing_tid(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t max_overlap, int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr,
                       uint32_t* cl, int32_t* n_found)
{
    ClipArrays A;
    const int rc = resident_clip(ctx, tid, &A);
    return rc ? rc : facing_arrays(ctx, "im_clip_facing_tid", A, min_reads, max_overlap, cap, pr, pl, cr, cl, n_found);
}

int im_clip_facing(im_ctx* ctx, int32_t min_reads, int32_t max_overlap, int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr, uint32_t* cl,
                   int32_t* n_found)
{
    ClipArrays A;
    const int rc = built_clip(ctx, "im_clip_facing", nullptr, &A);
    return rc ? rc : facing_arrays(ctx, "im_clip_facing", A, min_reads, max_overlap, cap, pr, pl, cr, cl, n_found);
}

// ---- clip tails: the clipped bases of clipped reads against the reference behind the partner breakpoint ----------

int im_cliptail_enable(im_ctx* ctx, int32_t min_clip, int32_t min_mapq, int32_t log2_slots) { return keyed_enable(ctx, &im_ctx::tail, &min_clip, min_mapq, log2_slots); }

int im_dev_cliptail_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream)
{
    return keyed_scatter(ctx, &im_ctx::tail, recs, stream, [](const im::RefDev& ref, const KeyedMember& T, const im_dev_records& r, hipStream_t st) {
        return im::launch_cliptail_scatter(ref, T.min_clip, T.min_mapq, r, T, st); });
}

// the host names the entries: checked here, staged through the workspace, one lane inserts each, wait
int im_cliptail_add(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* pos, const uint8_t* side, const uint8_t* nbases, const uint32_t* planes)
{
    if (!ctx || n < 0 || (n > 0 && (!pos || !side || !nbases || !planes))) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->tail, &tid);
    if (rc) return rc;
    for (int32_t i = 0; i < n; i++) {
        if (side[i] > 1) { set_err(ctx, "im_cliptail_add: entry %d: side %d, must be 0 (right) or 1 (left)", i, (int)side[i]); return IM_E_ARG; }
        if (nbases[i] < 1 || nbases[i] > 32) { set_err(ctx, "im_cliptail_add: entry %d: %d bases, must be 1 .. 32", i, (int)nbases[i]); return IM_E_ARG; }
    }
    if (n == 0) return IM_OK;
    WsColumns C;                                                    // pos, planes (two words per entry: two columns), side, bases
    rc = ws_columns(ctx, n, 5, &C);
    if (rc || (rc = C.down(0, pos, 4)) || (rc = C.down(1, planes, 8)) || (rc = C.down(3, side, 1)) || (rc = C.down(4, nbases, 1))) return rc;
    HIP_TRY(ctx, im::launch_cliptail_add(n, tid, ctx->h_len[tid], C.at<int32_t>(0), C.at<uint8_t>(3), C.at<uint8_t>(4), C.at<uint32_t>(1), ctx->tail, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return IM_OK;
}

// [pr][pl] in, one launch, the five answers and the two counters back, one wait; after an overflow every answer is "none"
int im_cliptail_verify(im_ctx* ctx, int32_t tid, int32_t nq, const int32_t* pr, const int32_t* pl, int32_t max_shift, uint32_t* v_right,
                       uint32_t* v_left, int32_t* shift, uint32_t* stored_right, uint32_t* stored_left)
{
    if (!ctx || nq < 0) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->tail, &tid);
    if (rc) return rc;
    if (max_shift < 0 || max_shift > 32) { set_err(ctx, "im_cliptail_verify: max_shift %d, must be 0 .. 32", max_shift); return IM_E_ARG; }
    if (nq == 0) return IM_OK;
    if (!pr || !pl || !v_right || !v_left || !shift || !stored_right || !stored_left) return IM_E_ARG;
    WsColumns C;                                                    // pr, pl, then the five answers
    rc = ws_columns(ctx, nq, 7, &C);
    if (rc || (rc = C.down(0, pr, 4)) || (rc = C.down(1, pl, 4))) return rc;
    HIP_TRY(ctx, im::launch_cliptail_verify(nq, tid, C.at<int32_t>(0), C.at<int32_t>(1), max_shift, ctx->ref_ascii + ctx->h_asc_off[tid], ctx->h_len[tid], ctx->tail,
                                            C.at<uint32_t>(2), C.at<uint32_t>(3), C.at<int32_t>(4), C.at<uint32_t>(5), C.at<uint32_t>(6), ctx->stream));
    return keyed_answers(ctx, ctx->tail, C, 2, {{v_right, 4}, {v_left, 4}, {shift, 4}, {stored_right, 4}, {stored_left, 4}});
}

// [pos][side] in, one launch, the five words per query and the two counters back, one wait; after an overflow every answer is "none"
int im_cliptail_consensus(im_ctx* ctx, int32_t tid, int32_t nq, const int32_t* pos, const uint8_t* side, int32_t min_cover, uint32_t* entries,
                          uint32_t* len, uint32_t* planes, uint32_t* agree)
{
    if (!ctx || nq < 0) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->tail, &tid);
    if (rc) return rc;
    if (min_cover < 1) { set_err(ctx, "im_cliptail_consensus: min_cover %d, must be >= 1", min_cover); return IM_E_ARG; }
    if (nq == 0) return IM_OK;
    if (!pos || !side || !entries || !len || !planes || !agree) return IM_E_ARG;
    for (int32_t q = 0; q < nq; q++) if (side[q] > 1) { set_err(ctx, "im_cliptail_consensus: query %d: side %d, must be 0 (right) or 1 (left)", q, (int)side[q]); return IM_E_ARG; }
    WsColumns C;                                                    // pos, side, entries, len, agree, planes (two words per query)
    rc = ws_columns(ctx, nq, 7, &C);
    if (rc || (rc = C.down(0, pos, 4)) || (rc = C.down(1, side, 1))) return rc;
    HIP_TRY(ctx, im::launch_cliptail_consensus(nq, tid, C.at<int32_t>(0), C.at<uint8_t>(1), min_cover, ctx->h_len[tid], ctx->tail, C.at<uint32_t>(2),
                                               C.at<uint32_t>(3), C.at<uint32_t>(5), C.at<uint32_t>(4), ctx->stream));
    return keyed_answers(ctx, ctx->tail, C, 2, {{entries, 4}, {len, 4}, {agree, 4}, {planes, 8}});
}

// ---- the peaks of either clip array, which the searches for pairs of piles start from ----------

static int peaks_args(im_ctx* ctx, const char* who, int32_t min_reads, int32_t reach, int32_t cap)
{
    if (min_reads < 1) { set_err(ctx, "%s: min_reads %d, must be >= 1", who, min_reads); return IM_E_ARG; }
    if (reach < 0 || reach > 64) { set_err(ctx, "%s: reach %d, must be 0 .. 64", who, reach); return IM_E_ARG; }
    if (cap < 0) { set_err(ctx, "%s: cap %d, must be >= 0", who, cap); return IM_E_ARG; }
    return IM_OK;
}

// (position, count) pairs from two device arrays of n, sorted by position (a position is a peak once)
static int sorted_peaks(im_ctx* ctx, void* d_pos, void* d_cnt, uint32_t n, std::vector<int32_t>& pos, std::vector<uint32_t>& cnt)
{
    pos.resize(n); cnt.resize(n);
    void* const d_col[2] = {d_pos, d_cnt};
    void* const out[2] = {pos.data(), cnt.data()};
    return sorted_columns(ctx, 2, d_col, n, {0}, out);
}

// the peaks of one contig's one array: the counter and two arrays of cap in the workspace, one launch, the counter back, then what
// was found, sorted by position here
static int peaks_array(im_ctx* ctx, const char* who, const ClipArrays& A, int32_t side, int32_t min_reads, int32_t reach, int32_t cap, int32_t* pos,
                       uint32_t* count, int32_t* n_found)
{
    if (side < 0 || side > 1) { set_err(ctx, "%s: side %d, must be 0 (right) or 1 (left)", who, side); return IM_E_ARG; }
    int rc = peaks_args(ctx, who, min_reads, reach, cap);
    if (rc) return rc;
    if (!n_found || (cap > 0 && (!pos || !count))) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t sb = up256(sizeof(int32_t) * (size_t)(cap ? cap : 1));
    rc = ensure_ws(ctx, 256 + 2 * sb);
    if (rc) return rc;
    uint32_t* d_count = (uint32_t*)ctx->ws;
    void* const d_col[2] = {(char*)ctx->ws + 256, (char*)ctx->ws + 256 + sb};
    uint32_t found = 0;
    HIP_TRY(ctx, im::launch_clip_peaks(side ? A.left : A.right, A.clen, min_reads, reach, cap, (int32_t*)d_col[0], (uint32_t*)d_col[1], d_count, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&found, d_count, sizeof found, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *n_found = (int32_t)found;
    if (found > (uint32_t)cap) return IM_OK;                        // more than cap: the caller asks again
    void* const out[2] = {pos, count};
    return sorted_columns(ctx, 2, d_col, found, {0}, out);
}

int im_clip_peaks_tid(im_ctx* ctx, int32_t tid, int32_t side, int32_t min_reads, int32_t reach, int32_t cap, int32_t* pos, uint32_t* count, int32_t* n_found)
{
    ClipArrays A;
    const int rc = resident_clip(ctx, tid, &A);
    return rc ? rc : peaks_array(ctx, "im_clip_peaks_tid", A, side, min_reads, reach, cap, pos, count, n_found);
}

int im_clip_peaks(im_ctx* ctx, int32_t side, int32_t min_reads, int32_t reach, int32_t cap, int32_t* pos, uint32_t* count, int32_t* n_found)
{
    ClipArrays A;
    const int rc = built_clip(ctx, "im_clip_peaks", nullptr, &A);
    return rc ? rc : peaks_array(ctx, "im_clip_peaks", A, side, min_reads, reach, cap, pos, count, n_found);
}

// The peaks of both arrays of one contig in the workspace: the counter block (256 bytes: the two peak counters, then the caller's
// pair counter), four lists of pb bytes (right positions, right counts, left positions, left counts), then out_bytes for the caller.
// Both peak passes, their two counters back, once more with room for all when a list did not fit.  found: the peaks per side.
struct PeakLists { char* base; size_t pb; uint32_t found[2]; };

static int peak_lists(im_ctx* ctx, const ClipArrays& A, int32_t min_reads, int32_t reach, size_t out_bytes, PeakLists* P)
{
    uint32_t pcap = 65536;
    for (;;) {
        P->pb = up256(sizeof(int32_t) * (size_t)pcap);
        int rc = ensure_ws(ctx, 256 + 4 * P->pb + out_bytes);
        if (rc) return rc;
        P->base = (char*)ctx->ws;
        uint32_t* d_count = (uint32_t*)P->base;
        HIP_TRY(ctx, im::launch_clip_peaks(A.right, A.clen, min_reads, reach, (int32_t)pcap, (int32_t*)(P->base + 256), (uint32_t*)(P->base + 256 + P->pb), d_count, ctx->stream));
        HIP_TRY(ctx, im::launch_clip_peaks(A.left, A.clen, min_reads, reach, (int32_t)pcap, (int32_t*)(P->base + 256 + 2 * P->pb), (uint32_t*)(P->base + 256 + 3 * P->pb), d_count + 1, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(P->found, d_count, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (P->found[0] <= pcap && P->found[1] <= pcap) return IM_OK;
        pcap = P->found[0] > P->found[1] ? P->found[0] : P->found[1];       // a list did not fit: once more, with room for all
    }
}

// the two lists down, SORTED HERE (piles are few) and up again; hp, hc: the host copies, which the uploads read until the next wait
static int sort_peak_lists(im_ctx* ctx, const PeakLists& P, void* d_list[4], std::vector<int32_t> hp[2], std::vector<uint32_t> hc[2])
{
    for (int k = 0; k < 4; k++) d_list[k] = P.base + 256 + k * P.pb;
    for (int k = 0; k < 2; k++) {
        int rc = sorted_peaks(ctx, d_list[2 * k], d_list[2 * k + 1], P.found[k], hp[k], hc[k]);
        if (rc) return rc;
        if (P.found[k] == 0) continue;
        HIP_TRY(ctx, hipMemcpyAsync(d_list[2 * k], hp[k].data(), sizeof(int32_t) * (size_t)P.found[k], hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_list[2 * k + 1], hc[k].data(), sizeof(uint32_t) * (size_t)P.found[k], hipMemcpyHostToDevice, ctx->stream));
    }
    return IM_OK;
}

// ---- pairs of piles: crossed, which a tandem duplication leaves (-U), and inverted, which an inversion's junction leaves (-N) ----------

// The pairs of piles of one contig, crossed (a right peak with the left peaks in front of it) or inverted (two peaks of one list).
// Behind the arguments, the table and the reference, in order: the table's counters (an overflowed table answers nothing), both peak
// passes into the workspace, their two counters back (peak_lists), the lists down, sorted and up again (sort_peak_lists), the ONE
// launch, its counter back, then min(found, cap) rows of ten columns down and sorted by (p1, p2, side) -- side is 0 in every crossed
// row.  side: the caller's side column (inverted) or null (crossed); out: p1, p2, c1, c2, v1, v2, shift, stored1, stored2.  The crossed
// search carries the side column too -- ten columns of workspace where it had nine, and a column of zeros brought down and dropped --
// so that one launch, one layout and one key list serve both kinds.
static int pile_pairs_arrays(im_ctx* ctx, const char* who, bool inverted, const ClipArrays& C, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len,
                             int32_t max_len, int32_t max_shift, int32_t min_verified, int32_t cap, uint8_t* side, void* const out[9], int32_t* n_found)
{
    int rc = keyed_ready(ctx, ctx->tail, nullptr);
    if (rc) return rc;
    if (!ctx->ref_ascii) { set_err(ctx, "im_set_reference has not been called"); return IM_E_ARG; }
    if ((rc = peaks_args(ctx, who, min_reads, reach, cap))) return rc;
    if (min_len < 1) { set_err(ctx, "%s: min_len %d, must be >= 1", who, min_len); return IM_E_ARG; }
    if (max_len < min_len) { set_err(ctx, "%s: max_len %d, must be >= min_len %d", who, max_len, min_len); return IM_E_ARG; }
    if (max_shift < 0 || max_shift > 32) { set_err(ctx, "%s: max_shift %d, must be 0 .. 32", who, max_shift); return IM_E_ARG; }
    if (min_verified < 1) { set_err(ctx, "%s: min_verified %d, must be >= 1", who, min_verified); return IM_E_ARG; }
    bool all = n_found && (!inverted || cap == 0 || side);
    for (int k = 0; k < 9; k++) all = all && (cap == 0 || out[k]);
    if (!all) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    bool over = false;
    rc = keyed_overflowed(ctx, ctx->tail, &over);
    if (rc) return rc;
    if (over) { *n_found = -1; return IM_OK; }
    const size_t ob = up256(sizeof(int32_t) * (size_t)(cap ? cap : 1));
    PeakLists P;
    rc = peak_lists(ctx, C, min_reads, reach, 10 * ob, &P);
    if (rc) return rc;
    *n_found = 0;
    // crossed: a pair takes a peak of either list; inverted: two peaks of one list
    if (inverted ? P.found[0] < 2 && P.found[1] < 2 : P.found[0] == 0 || P.found[1] == 0) return IM_OK;
    void* d_list[4];
    std::vector<int32_t> hp[2];
    std::vector<uint32_t> hc[2];
    rc = sort_peak_lists(ctx, P, d_list, hp, hc);
    if (rc) return rc;
    void* d_out[10];
    for (int k = 0; k < 10; k++) d_out[k] = P.base + 256 + 4 * P.pb + k * ob;
    im::TailPairsArgs A;
    A.n_right = (int32_t)P.found[0]; A.n_left = (int32_t)P.found[1]; A.tid = tid;
    A.rpos = (const int32_t*)d_list[0]; A.rcnt = (const uint32_t*)d_list[1]; A.lpos = (const int32_t*)d_list[2]; A.lcnt = (const uint32_t*)d_list[3];
    A.min_len = min_len; A.max_len = max_len; A.max_shift = max_shift; A.min_verified = min_verified; A.cap = cap;
    A.ref = ctx->ref_ascii + ctx->h_asc_off[tid]; A.clen = ctx->h_len[tid]; A.tab = ctx->tail;
    for (int k = 0; k < 10; k++) A.col[k] = (uint32_t*)d_out[k];
    A.n_found = (uint32_t*)P.base + 2;
    uint32_t found = 0;
    HIP_TRY(ctx, im::launch_cliptail_pairs(inverted, A, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&found, A.n_found, sizeof found, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));                // the uploads' host vectors are done with here as well
    *n_found = (int32_t)found;
    const uint32_t n = found < (uint32_t)cap ? found : (uint32_t)cap;
    std::vector<int32_t> hside(n);                                  // a word per row here, a byte per row (or nothing) at the caller
    void* const h_out[10] = {hside.data(), out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7], out[8]};
    rc = sorted_columns(ctx, 10, d_out, n, {1, 2, 0}, h_out);
    for (uint32_t i = 0; i < n && side && !rc; i++) side[i] = (uint8_t)hside[i];
    return rc;
}

int im_clip_crossed_tid(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift, int32_t min_verified,
                        int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr, uint32_t* cl, uint32_t* v_right, uint32_t* v_left, int32_t* shift,
                        uint32_t* stored_right, uint32_t* stored_left, int32_t* n_found)
{
    ClipArrays A;
    void* const out[9] = {pr, pl, cr, cl, v_right, v_left, shift, stored_right, stored_left};
    const int rc = resident_clip(ctx, tid, &A);
    return rc ? rc : pile_pairs_arrays(ctx, "im_clip_crossed_tid", false, A, tid, min_reads, reach, min_len, max_len, max_shift, min_verified, cap, nullptr, out, n_found);
}

int im_clip_crossed(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift, int32_t min_verified,
                    int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr, uint32_t* cl, uint32_t* v_right, uint32_t* v_left, int32_t* shift,
                    uint32_t* stored_right, uint32_t* stored_left, int32_t* n_found)
{
    ClipArrays A;
    void* const out[9] = {pr, pl, cr, cl, v_right, v_left, shift, stored_right, stored_left};
    const int rc = built_clip(ctx, "im_clip_crossed", &tid, &A);
    return rc ? rc : pile_pairs_arrays(ctx, "im_clip_crossed", false, A, tid, min_reads, reach, min_len, max_len, max_shift, min_verified, cap, nullptr, out, n_found);
}

int im_clip_inverted_tid(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift, int32_t min_verified,
                         int32_t cap, uint8_t* side, int32_t* p1, int32_t* p2, uint32_t* c1, uint32_t* c2, uint32_t* v1, uint32_t* v2, int32_t* shift,
                         uint32_t* stored1, uint32_t* stored2, int32_t* n_found)
{
    ClipArrays A;
    void* const out[9] = {p1, p2, c1, c2, v1, v2, shift, stored1, stored2};
    const int rc = resident_clip(ctx, tid, &A);
    return rc ? rc : pile_pairs_arrays(ctx, "im_clip_inverted_tid", true, A, tid, min_reads, reach, min_len, max_len, max_shift, min_verified, cap, side, out, n_found);
}

int im_clip_inverted(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift, int32_t min_verified,
                     int32_t cap, uint8_t* side, int32_t* p1, int32_t* p2, uint32_t* c1, uint32_t* c2, uint32_t* v1, uint32_t* v2, int32_t* shift,
                     uint32_t* stored1, uint32_t* stored2, int32_t* n_found)
{
    ClipArrays A;
    void* const out[9] = {p1, p2, c1, c2, v1, v2, shift, stored1, stored2};
    const int rc = built_clip(ctx, "im_clip_inverted", &tid, &A);
    return rc ? rc : pile_pairs_arrays(ctx, "im_clip_inverted", true, A, tid, min_reads, reach, min_len, max_len, max_shift, min_verified, cap, side, out, n_found);
}

int im_cliptail_reset(im_ctx* ctx, void* stream) { return keyed_reset(ctx, &im_ctx::tail, stream); }
int im_cliptail_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped) { return keyed_stats(ctx, &im_ctx::tail, stored, dropped); }

// ---- pair links: the read pairs of an abnormal orientation, counted between two windows (-M) ----------

int im_pairlink_enable(im_ctx* ctx, int32_t min_mapq, int32_t log2_slots) { return keyed_enable(ctx, &im_ctx::link, nullptr, min_mapq, log2_slots); }
int im_pairlink_reset(im_ctx* ctx, void* stream) { return keyed_reset(ctx, &im_ctx::link, stream); }
int im_pairlink_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped) { return keyed_stats(ctx, &im_ctx::link, stored, dropped); }

// in the stretched form, the kernel instantiation with the fourth kind; without, the one there was
int im_dev_pairlink_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream)
{
    return link_scatter(ctx, &im_ctx::link, recs, stream, ctx && ctx->link_stretched ? im::launch_pairlink_scatter_stretched : im::launch_pairlink_scatter);
}

// the host names the links: checked here, staged through the workspace, one lane inserts each, wait
int im_pairlink_add(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* pos, const int32_t* mpos, const uint8_t* kind)
{
    if (!ctx || n < 0 || (n > 0 && (!pos || !mpos || !kind))) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->link, &tid);
    if (rc || (rc = link_args(ctx, "im_pairlink_add", "link", ctx->link_stretched ? kPairKindsStretched : kPairKinds, n, kind, nullptr, nullptr))) return rc;
    if (n == 0) return IM_OK;
    WsColumns C;                                                    // pos, mpos, kind
    rc = ws_columns(ctx, n, 3, &C);
    if (rc || (rc = C.down(0, pos, 4)) || (rc = C.down(1, mpos, 4)) || (rc = C.down(2, kind, 1))) return rc;
    HIP_TRY(ctx, im::launch_pairlink_add(n, tid, ctx->h_len[tid], C.at<int32_t>(0), C.at<int32_t>(1), C.at<uint8_t>(2), ctx->link, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return IM_OK;
}

// [kind][a0][a1][b0][b1] in, one launch, the counts and the two counters back, one wait; after an overflow every answer is "none"
int im_pairlink_count(im_ctx* ctx, int32_t tid, int32_t nq, const uint8_t* kind, const int32_t* a0, const int32_t* a1, const int32_t* b0,
                      const int32_t* b1, int32_t min_sep, uint32_t* count_out)
{
    if (!ctx || nq < 0) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->link, &tid);
    if (rc) return rc;
    if (min_sep < 0) { set_err(ctx, "im_pairlink_count: min_sep %d, must be >= 0", min_sep); return IM_E_ARG; }
    if (nq == 0) return IM_OK;
    if (!kind || !a0 || !a1 || !b0 || !b1 || !count_out) return IM_E_ARG;
    if ((rc = link_args(ctx, "im_pairlink_count", "query", ctx->link_stretched ? kPairKindsStretched : kPairKinds, nq, kind, a0, a1))) return rc;
    WsColumns C;                                                    // a0, a1, b0, b1, kind, the counts
    rc = ws_columns(ctx, nq, 6, &C);
    const int32_t* h_in[4] = {a0, a1, b0, b1};
    for (int k = 0; k < 4 && !rc; k++) rc = C.down(k, h_in[k], 4);
    if (rc || (rc = C.down(4, kind, 1))) return rc;
    HIP_TRY(ctx, im::launch_pairlink_count(nq, tid, C.at<uint8_t>(4), C.at<int32_t>(0), C.at<int32_t>(1), C.at<int32_t>(2), C.at<int32_t>(3), min_sep, ctx->h_len[tid],
                                           ctx->link, C.at<uint32_t>(5), ctx->stream));
    return keyed_answers(ctx, ctx->link, C, 5, {{count_out, 4}});
}

// The fourth kind of the pair links (-E).  Behind im_pairlink_enable and in front of the first link: a pair delivered earlier would
// have stored no link although the rule now gives it one.
int im_pairlink_stretched_enable(im_ctx* ctx)
{
    if (!ctx) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->link, nullptr);
    if (rc) return rc;
    if (ctx->link_stretched) return IM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long counters[2] = {0, 0};
    if ((rc = keyed_counters(ctx, ctx->link, counters))) return rc;
    if (counters[0] > 0) {
        set_err(ctx, "im_pairlink_stretched_enable: %llu links have been asked for already; enable in front of the first (or behind im_pairlink_reset)", counters[0]);
        return IM_E_ARG;
    }
    ctx->link_stretched = true;
    return IM_OK;
}

// ---- mate links: the read pairs whose mate lies on another contig, asked where the mates of a window lie (-T) ----------

int im_matelink_enable(im_ctx* ctx, int32_t min_mapq, int32_t log2_slots) { return keyed_enable(ctx, &im_ctx::mate, nullptr, min_mapq, log2_slots); }
int im_matelink_reset(im_ctx* ctx, void* stream) { return keyed_reset(ctx, &im_ctx::mate, stream); }
int im_matelink_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped) { return keyed_stats(ctx, &im_ctx::mate, stored, dropped); }
int im_dev_matelink_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream) { return link_scatter(ctx, &im_ctx::mate, recs, stream, im::launch_matelink_scatter); }

// the host names the links: checked here, staged through the workspace, one lane inserts each, wait
int im_matelink_add(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* pos, const int32_t* mtid, const int32_t* mpos, const uint8_t* kind)
{
    if (!ctx || n < 0 || (n > 0 && (!pos || !mtid || !mpos || !kind))) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->mate, &tid);
    if (rc || (rc = link_args(ctx, "im_matelink_add", "link", kMateKinds, n, kind, nullptr, nullptr))) return rc;
    if (n == 0) return IM_OK;
    WsColumns C;                                                    // pos, mtid, mpos, kind
    rc = ws_columns(ctx, n, 4, &C);
    if (rc || (rc = C.down(0, pos, 4)) || (rc = C.down(1, mtid, 4)) || (rc = C.down(2, mpos, 4)) || (rc = C.down(3, kind, 1))) return rc;
    HIP_TRY(ctx, im::launch_matelink_add(ref_dev(ctx), n, tid, C.at<int32_t>(0), C.at<int32_t>(1), C.at<int32_t>(2), C.at<uint8_t>(3), ctx->mate, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return IM_OK;
}

// [kind][a0][a1] in, one launch, the five answers and the two counters back, one wait; after an overflow every answer is "none"
int im_matelink_partner(im_ctx* ctx, int32_t tid, int32_t nq, const uint8_t* kind, const int32_t* a0, const int32_t* a1, uint32_t* n_links,
                        int32_t* mtid_out, uint32_t* n_partner, int32_t* lo, int32_t* hi)
{
    if (!ctx || nq < 0) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->mate, &tid);
    if (rc) return rc;
    if (nq == 0) return IM_OK;
    if (!kind || !a0 || !a1 || !n_links || !mtid_out || !n_partner || !lo || !hi) return IM_E_ARG;
    if ((rc = link_args(ctx, "im_matelink_partner", "query", kMateKinds, nq, kind, a0, a1))) return rc;
    WsColumns C;                                                    // a0, a1, kind, then the five answers
    rc = ws_columns(ctx, nq, 8, &C);
    if (rc || (rc = C.down(0, a0, 4)) || (rc = C.down(1, a1, 4)) || (rc = C.down(2, kind, 1))) return rc;
    HIP_TRY(ctx, im::launch_matelink_partner(nq, tid, C.at<uint8_t>(2), C.at<int32_t>(0), C.at<int32_t>(1), ctx->h_len[tid], ctx->mate, C.at<uint32_t>(3),
                                             C.at<int32_t>(4), C.at<uint32_t>(5), C.at<int32_t>(6), C.at<int32_t>(7), ctx->stream));
    return keyed_answers(ctx, ctx->mate, C, 3, {{n_links, 4}, {mtid_out, 4}, {n_partner, 4}, {lo, 4}, {hi, 4}});
}

// ---- junction pairs: the read pairs on either side of a junction, out of both tables in one launch (-E) ----------

// six columns in, one launch, the two answers and both tables' counters back, one wait; a junction whose table has dropped links is "none"
int im_junction_pairs(im_ctx* ctx, int32_t n, const int32_t* tid1, const int32_t* pos1, const uint8_t* side1, const int32_t* tid2, const int32_t* pos2,
                      const uint8_t* side2, int32_t reach, int32_t back, int32_t min_sep, uint32_t* pe1, uint32_t* pe2)
{
    if (!ctx) return IM_E_ARG;
    const char* who = "im_junction_pairs";
    if (n < 0) { set_err(ctx, "%s: n %d, must be >= 0", who, n); return IM_E_ARG; }
    int rc = keyed_ready(ctx, ctx->link, nullptr);
    if (rc || (rc = keyed_ready(ctx, ctx->mate, nullptr))) return rc;
    if (!ctx->link_stretched) { set_err(ctx, "im_pairlink_stretched_enable has not been called"); return IM_E_ARG; }
    if (reach < 0 || back < 0 || (long long)reach + back > 65535) {
        set_err(ctx, "%s: reach %d, back %d, must be >= 0 and reach + back <= 65535", who, reach, back);
        return IM_E_ARG;
    }
    if (min_sep < 0) { set_err(ctx, "%s: min_sep %d, must be >= 0", who, min_sep); return IM_E_ARG; }
    if (n == 0) return IM_OK;
    if (!tid1 || !pos1 || !side1 || !tid2 || !pos2 || !side2 || !pe1 || !pe2) { set_err(ctx, "%s: junction 0: a null column with n %d", who, n); return IM_E_ARG; }
    if ((rc = split_sides(ctx, who, "junction", n, side1, side2))) return rc;
    for (int32_t k = 0; k < n; k++)
        if (tid1[k] < 0 || tid1[k] >= ctx->n_contigs || tid2[k] < 0 || tid2[k] >= ctx->n_contigs) {
            set_err(ctx, "%s: junction %d: contigs %d and %d, must be 0 .. %d", who, k, tid1[k], tid2[k], ctx->n_contigs - 1);
            return IM_E_ARG;
        }
    WsColumns C;                                                    // tid1, pos1, tid2, pos2, side1, side2, then the two answers
    rc = ws_columns(ctx, n, 8, &C);
    const int32_t* h_in[4] = {tid1, pos1, tid2, pos2};
    for (int k = 0; k < 4 && !rc; k++) rc = C.down(k, h_in[k], 4);
    if (rc || (rc = C.down(4, side1, 1)) || (rc = C.down(5, side2, 1))) return rc;
    im::JuncPairArgs A;
    A.nq = n; A.reach = reach; A.back = back; A.min_sep = min_sep; A.tid1 = C.at<int32_t>(0); A.pos1 = C.at<int32_t>(1); A.side1 = C.at<uint8_t>(4);
    A.tid2 = C.at<int32_t>(2); A.pos2 = C.at<int32_t>(3); A.side2 = C.at<uint8_t>(5); A.len = ctx->d_len; A.pair = ctx->link; A.mate = ctx->mate;
    A.pe1 = C.at<uint32_t>(6); A.pe2 = C.at<uint32_t>(7);
    HIP_TRY(ctx, im::launch_junction_pairs(A, ctx->stream));
    // the answers and the counters of both tables behind the launch, one wait; the overflow is per table: a junction on one contig is
    // blanked by the pair links' drops, one on two contigs by the mate links'
    unsigned long long pair_counters[2] = {0, 0}, mate_counters[2] = {0, 0};
    if ((rc = C.up(6, pe1, 4)) || (rc = C.up(7, pe2, 4))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(pair_counters, ctx->link.counters, sizeof pair_counters, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = keyed_counters(ctx, ctx->mate, mate_counters))) return rc;
    const bool pair_over = pair_counters[1] > 0, mate_over = mate_counters[1] > 0;
    for (int32_t k = 0; k < n && (pair_over || mate_over); k++)
        if (tid1[k] == tid2[k] ? pair_over : mate_over) pe1[k] = pe2[k] = 0xFFFFFFFFu;
    return IM_OK;
}

// ---- split links: the soft-clipped primary records whose SA:Z tag places the clipped part, counted between two junction ends (-S) ----------

int im_splitlink_enable(im_ctx* ctx, int32_t min_clip, int32_t min_mapq, int32_t log2_slots, int32_t n_names, const char* const* names)
{
    if (!ctx) return IM_E_ARG;
    if (!ctx->ref_ascii) { set_err(ctx, "im_set_reference has not been called"); return IM_E_ARG; }
    if (n_names != ctx->n_contigs || !names) { set_err(ctx, "im_splitlink_enable: %d names for %d contigs", names ? n_names : 0, ctx->n_contigs); return IM_E_ARG; }
    std::vector<std::string> list;
    std::unordered_map<std::string, int32_t> seen;
    for (int32_t i = 0; i < n_names; i++) {
        if (!names[i] || !names[i][0]) { set_err(ctx, "im_splitlink_enable: name %d is null or empty", i); return IM_E_ARG; }
        const auto ins = seen.emplace(names[i], i);
        if (!ins.second) { set_err(ctx, "im_splitlink_enable: names %d and %d are equal (%s)", ins.first->second, i, names[i]); return IM_E_ARG; }
        list.emplace_back(names[i]);
    }
    if (ctx->split.slots) {
        if (list != ctx->split_names) { set_err(ctx, "im_splitlink_enable: already enabled with other contig names"); return IM_E_ARG; }
        return keyed_enable(ctx, &im_ctx::split, &min_clip, min_mapq, log2_slots);      // the same values again, or the refusal
    }
    const int rc = keyed_enable(ctx, &im_ctx::split, &min_clip, min_mapq, log2_slots);
    if (rc) return rc;
    const std::vector<uint8_t> blob = split_name_blob(list);
    hipError_t e = hipMalloc((void**)&ctx->split_blob, blob.size());
    if (e == hipSuccess) e = hipMemcpy(ctx->split_blob, blob.data(), blob.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        // no table without its names
        if (ctx->split_blob) (void)hipFree(ctx->split_blob);
        (void)hipFree(ctx->split.slots); (void)hipFree(ctx->split.counters);
        ctx->split = KeyedMember(ctx->split.enable); ctx->split_blob = nullptr;
        set_err(ctx, "im_splitlink_enable: the name table: %s", hipGetErrorString(e));
        return IM_E_HIP;
    }
    ctx->split_names = list;
    return IM_OK;
}

// the overlap array goes back to "unknown" with the slots it belongs to
int im_splitlink_reset(im_ctx* ctx, void* stream)
{
    const int rc = keyed_reset(ctx, &im_ctx::split, stream);
    if (rc || !ctx->split_ovl) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->split_ovl, 0, (size_t)2 << ctx->split.log2_slots, (hipStream_t)stream));
    return IM_OK;
}

int im_splitlink_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped) { return keyed_stats(ctx, &im_ctx::split, stored, dropped); }

// with the overlap array on, the kernel instantiation that fills it; without, the one there was
int im_dev_splitlink_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream)
{
    const uint8_t* names = ctx ? ctx->split_blob : nullptr;
    uint16_t* ovl = ctx ? ctx->split_ovl : nullptr;
    return keyed_scatter(ctx, &im_ctx::split, recs, stream, [names, ovl](const im::RefDev& ref, const KeyedMember& T, const im_dev_records& r, hipStream_t st) {
        return ovl ? im::launch_splitlink_scatter_overlap(ref, T.min_clip, T.min_mapq, names, r, T, ovl, st)
                   : im::launch_splitlink_scatter(ref, T.min_clip, T.min_mapq, names, r, T, st); });
}

// the host names the links: checked here, staged through the workspace, one lane inserts each, wait
int im_splitlink_add(im_ctx* ctx, int32_t n, const int32_t* tid, const int32_t* pos, const uint8_t* side, const int32_t* tid2, const int32_t* pos2,
                     const uint8_t* side2)
{
    if (!ctx || n < 0 || (n > 0 && (!tid || !pos || !side || !tid2 || !pos2 || !side2))) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->split, nullptr);
    if (rc || (rc = split_sides(ctx, "im_splitlink_add", "link", n, side, side2))) return rc;
    if (n == 0) return IM_OK;
    WsColumns C;                                                    // tid, pos, tid2, pos2, side, side2
    rc = ws_columns(ctx, n, 6, &C);
    const int32_t* h_in[4] = {tid, pos, tid2, pos2};
    for (int k = 0; k < 4 && !rc; k++) rc = C.down(k, h_in[k], 4);
    if (rc || (rc = C.down(4, side, 1)) || (rc = C.down(5, side2, 1))) return rc;
    HIP_TRY(ctx, im::launch_splitlink_add(ref_dev(ctx), n, C.at<int32_t>(0), C.at<int32_t>(1), C.at<uint8_t>(4), C.at<int32_t>(2), C.at<int32_t>(3),
                                          C.at<uint8_t>(5), ctx->split, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return IM_OK;
}

// eight columns in, one launch, the counts and the two counters back, one wait; after an overflow every answer is "none"
int im_splitlink_count(im_ctx* ctx, int32_t nq, const int32_t* tid1, const uint8_t* side1, const int32_t* a0, const int32_t* a1, const int32_t* tid2,
                       const uint8_t* side2, const int32_t* b0, const int32_t* b1, uint32_t* count_out)
{
    if (!ctx || nq < 0) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->split, nullptr);
    if (rc) return rc;
    if (nq == 0) return IM_OK;
    if (!tid1 || !side1 || !a0 || !a1 || !tid2 || !side2 || !b0 || !b1 || !count_out) return IM_E_ARG;
    if ((rc = split_sides(ctx, "im_splitlink_count", "query", nq, side1, side2))) return rc;
    for (int32_t q = 0; q < nq; q++) {
        if (tid1[q] < 0 || tid1[q] >= ctx->n_contigs || tid2[q] < 0 || tid2[q] >= ctx->n_contigs) {
            set_err(ctx, "im_splitlink_count: query %d: contigs %d and %d, must be 0 .. %d", q, tid1[q], tid2[q], ctx->n_contigs - 1);
            return IM_E_ARG;
        }
        const long long span = (long long)a1[q] - (long long)a0[q];
        if (span > 65535) { set_err(ctx, "im_splitlink_count: query %d: a1 - a0 = %lld, must be <= 65535", q, span); return IM_E_ARG; }
    }
    WsColumns C;                                                    // tid1, a0, a1, tid2, b0, b1, side1, side2, the counts
    rc = ws_columns(ctx, nq, 9, &C);
    const int32_t* h_in[6] = {tid1, a0, a1, tid2, b0, b1};
    for (int k = 0; k < 6 && !rc; k++) rc = C.down(k, h_in[k], 4);
    if (rc || (rc = C.down(6, side1, 1)) || (rc = C.down(7, side2, 1))) return rc;
    HIP_TRY(ctx, im::launch_splitlink_count(ref_dev(ctx), nq, C.at<int32_t>(0), C.at<uint8_t>(6), C.at<int32_t>(1), C.at<int32_t>(2), C.at<int32_t>(3),
                                            C.at<uint8_t>(7), C.at<int32_t>(4), C.at<int32_t>(5), ctx->split, C.at<uint32_t>(8), ctx->stream));
    return keyed_answers(ctx, ctx->split, C, 8, {{count_out, 4}});
}

// The junctions of the table alone.  The table's counters first: after an overflow there is no answer, and counters[0] is the list's
// length.  The workspace is this call's own (12 bytes per stored link, 4 per slot, the nine columns), allocated here and freed here: the
// call is made once per run.  Three launches, the count back, then -- when it fits cap -- the columns, sorted here by (tid1, pos1, tid2,
// pos2, side1, side2).
int im_splitlink_junctions(im_ctx* ctx, int32_t window, int32_t min_links, int32_t min_span, int32_t cap, int32_t* tid1, int32_t* pos1, uint8_t* side1,
                           int32_t* tid2, int32_t* pos2, uint8_t* side2, uint32_t* exact, uint32_t* n1, uint32_t* n2, int32_t* found)
{
    if (!ctx) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->split, nullptr);
    if (rc) return rc;
    const char* who = "im_splitlink_junctions";
    if (window < 0 || window > 255) { set_err(ctx, "%s: window %d, must be 0 .. 255", who, window); return IM_E_ARG; }
    if (min_links < 1) { set_err(ctx, "%s: min_links %d, must be >= 1", who, min_links); return IM_E_ARG; }
    if (min_span < 0) { set_err(ctx, "%s: min_span %d, must be >= 0", who, min_span); return IM_E_ARG; }
    if (cap < 0) { set_err(ctx, "%s: cap %d, must be >= 0", who, cap); return IM_E_ARG; }
    if (!found) { set_err(ctx, "%s: found is null", who); return IM_E_ARG; }
    if (cap > 0 && (!tid1 || !pos1 || !side1 || !tid2 || !pos2 || !side2 || !exact || !n1 || !n2)) { set_err(ctx, "%s: a null column with cap %d", who, cap); return IM_E_ARG; }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long counters[2] = {0, 0};
    if ((rc = keyed_counters(ctx, ctx->split, counters))) return rc;
    if (counters[1] > 0) { *found = -1; return IM_OK; }
    *found = 0;
    if (counters[0] == 0) return IM_OK;
    const size_t n_list = (size_t)counters[0], slots = (size_t)1 << ctx->split.log2_slots;
    const size_t lb = up256(sizeof(uint32_t) * n_list), eb = up256(sizeof(uint32_t) * slots), cb = up256(sizeof(uint32_t) * (size_t)(cap ? cap : 1));
    char* ws = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&ws, 256 + 3 * lb + eb + 9 * cb));
    im::SplitJuncArgs A;
    A.tab = ctx->split; A.len = ctx->d_len; A.window = window; A.min_links = min_links; A.min_span = min_span; A.cap = cap; A.n_list = (uint32_t)n_list;
    A.counters = (unsigned long long*)ws;
    A.list = (uint32_t*)(ws + 256); A.n_own = (uint32_t*)(ws + 256 + lb); A.n_far = (uint32_t*)(ws + 256 + 2 * lb); A.exact = (uint32_t*)(ws + 256 + 3 * lb);
    for (int k = 0; k < 9; k++) A.col[k] = (uint32_t*)(ws + 256 + 3 * lb + eb + k * cb);
    unsigned long long got[2] = {0, 0};
    hipError_t e = im::launch_splitlink_junctions(A, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(got, A.counters, sizeof got, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    const size_t n = (size_t)got[1];
    std::vector<uint32_t> h(n <= (size_t)cap ? 9 * n : 0);
    if (e == hipSuccess && n > 0 && n <= (size_t)cap) {
        for (int k = 0; k < 9 && e == hipSuccess; k++) e = hipMemcpyAsync(h.data() + k * n, A.col[k], sizeof(uint32_t) * n, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    const hipError_t ef = hipFree(ws);
    if (e == hipSuccess) e = ef;
    if (e != hipSuccess) { set_err(ctx, "%s: %s", who, hipGetErrorString(e)); return IM_E_HIP; }
    *found = (int32_t)n;
    if (n == 0 || n > (size_t)cap) return IM_OK;
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
    const int by[6] = {0, 1, 3, 4, 2, 5};                           // the driver's record order: tid1, pos1, tid2, pos2, side1, side2
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        for (int k : by) if (h[k * n + a] != h[k * n + b]) return h[k * n + a] < h[k * n + b];
        return false;
    });
    for (size_t i = 0; i < n; i++) {
        const uint32_t r = order[i];
        tid1[i] = (int32_t)h[r]; pos1[i] = (int32_t)h[n + r]; side1[i] = (uint8_t)h[2 * n + r];
        tid2[i] = (int32_t)h[3 * n + r]; pos2[i] = (int32_t)h[4 * n + r]; side2[i] = (uint8_t)h[5 * n + r];
        exact[i] = h[6 * n + r]; n1[i] = h[7 * n + r]; n2[i] = h[8 * n + r];
    }
    return IM_OK;
}

// ---- junction overlap: micro-homology and inserted bases of the split links, summed up per junction (-H) ----------

// The array beside the table: a 16-bit code per slot, zero = unknown.  Behind im_splitlink_enable and in front of the first link: a
// link stored earlier would have no d although its record had one.
int im_splitlink_overlap_enable(im_ctx* ctx)
{
    if (!ctx) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->split, nullptr);
    if (rc) return rc;
    if (ctx->split_ovl) return IM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long counters[2] = {0, 0};
    if ((rc = keyed_counters(ctx, ctx->split, counters))) return rc;
    if (counters[0] > 0) {
        set_err(ctx, "im_splitlink_overlap_enable: %llu links have been asked for already; enable in front of the first (or behind im_splitlink_reset)", counters[0]);
        return IM_E_ARG;
    }
    const size_t bytes = (size_t)2 << ctx->split.log2_slots;
    uint16_t* ovl = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&ovl, bytes));
    hipError_t e = hipMemsetAsync(ovl, 0, bytes, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipFree(ovl); set_err(ctx, "im_splitlink_overlap_enable: %s", hipGetErrorString(e)); return IM_E_HIP; }
    ctx->split_ovl = ovl;
    return IM_OK;
}

// im_splitlink_add with a seventh column
int im_splitlink_add_overlap(im_ctx* ctx, int32_t n, const int32_t* tid, const int32_t* pos, const uint8_t* side, const int32_t* tid2, const int32_t* pos2,
                             const uint8_t* side2, const int16_t* d)
{
    if (!ctx || n < 0 || (n > 0 && (!tid || !pos || !side || !tid2 || !pos2 || !side2 || !d))) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->split, nullptr);
    if (rc) return rc;
    if (!ctx->split_ovl) { set_err(ctx, "im_splitlink_overlap_enable has not been called"); return IM_E_ARG; }
    if ((rc = split_sides(ctx, "im_splitlink_add_overlap", "link", n, side, side2))) return rc;
    if (n == 0) return IM_OK;
    WsColumns C;                                                    // tid, pos, tid2, pos2, side, side2, d
    rc = ws_columns(ctx, n, 7, &C);
    const int32_t* h_in[4] = {tid, pos, tid2, pos2};
    for (int k = 0; k < 4 && !rc; k++) rc = C.down(k, h_in[k], 4);
    if (rc || (rc = C.down(4, side, 1)) || (rc = C.down(5, side2, 1)) || (rc = C.down(6, d, 2))) return rc;
    HIP_TRY(ctx, im::launch_splitlink_add_overlap(ref_dev(ctx), n, C.at<int32_t>(0), C.at<int32_t>(1), C.at<uint8_t>(4), C.at<int32_t>(2), C.at<int32_t>(3),
                                                  C.at<uint8_t>(5), C.at<int16_t>(6), ctx->split, ctx->split_ovl, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return IM_OK;
}

// six columns in, one launch, the three answers and the two counters back, one wait; after an overflow every answer is "none"
int im_splitlink_overlap(im_ctx* ctx, int32_t n, const int32_t* tid1, const int32_t* pos1, const uint8_t* side1, const int32_t* tid2, const int32_t* pos2,
                         const uint8_t* side2, int32_t window, uint32_t* known, int32_t* median, uint32_t* agree)
{
    if (!ctx || n < 0) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->split, nullptr);
    if (rc) return rc;
    const char* who = "im_splitlink_overlap";
    if (!ctx->split_ovl) { set_err(ctx, "im_splitlink_overlap_enable has not been called"); return IM_E_ARG; }
    if (window < 0 || window > 255) { set_err(ctx, "%s: window %d, must be 0 .. 255", who, window); return IM_E_ARG; }
    if (n == 0) return IM_OK;
    if (!tid1 || !pos1 || !side1 || !tid2 || !pos2 || !side2 || !known || !median || !agree) return IM_E_ARG;
    if ((rc = split_sides(ctx, who, "junction", n, side1, side2))) return rc;
    for (int32_t k = 0; k < n; k++)
        if (tid1[k] < 0 || tid1[k] >= ctx->n_contigs || tid2[k] < 0 || tid2[k] >= ctx->n_contigs) {
            set_err(ctx, "%s: junction %d: contigs %d and %d, must be 0 .. %d", who, k, tid1[k], tid2[k], ctx->n_contigs - 1);
            return IM_E_ARG;
        }
    WsColumns C;                                                    // tid1, pos1, tid2, pos2, side1, side2, then the three answers
    rc = ws_columns(ctx, n, 9, &C);
    const int32_t* h_in[4] = {tid1, pos1, tid2, pos2};
    for (int k = 0; k < 4 && !rc; k++) rc = C.down(k, h_in[k], 4);
    if (rc || (rc = C.down(4, side1, 1)) || (rc = C.down(5, side2, 1))) return rc;
    im::SplitOverlapArgs A;
    A.nq = n; A.window = window; A.tid1 = C.at<int32_t>(0); A.pos1 = C.at<int32_t>(1); A.side1 = C.at<uint8_t>(4);
    A.tid2 = C.at<int32_t>(2); A.pos2 = C.at<int32_t>(3); A.side2 = C.at<uint8_t>(5); A.len = ctx->d_len; A.tab = ctx->split; A.ovl = ctx->split_ovl;
    A.known = C.at<uint32_t>(6); A.median = C.at<int32_t>(7); A.agree = C.at<uint32_t>(8);
    HIP_TRY(ctx, im::launch_splitlink_overlap(A, ctx->stream));
    return keyed_answers(ctx, ctx->split, C, 6, {{known, 4}, {median, 4}, {agree, 4}});
}

// six columns in, one launch, the five answers and the two counters back, one wait; after an overflow every answer is "none"
int im_cliptail_junction(im_ctx* ctx, int32_t nq, const int32_t* tid1, const int32_t* p1, const uint8_t* side1, const int32_t* tid2, const int32_t* p2,
                         const uint8_t* side2, int32_t max_shift, uint32_t* v1, uint32_t* v2, int32_t* shift, uint32_t* stored1, uint32_t* stored2)
{
    if (!ctx || nq < 0) return IM_E_ARG;
    int rc = keyed_ready(ctx, ctx->tail, nullptr);
    if (rc) return rc;
    if (max_shift < 0 || max_shift > 32) { set_err(ctx, "im_cliptail_junction: max_shift %d, must be 0 .. 32", max_shift); return IM_E_ARG; }
    if (nq == 0) return IM_OK;
    if (!tid1 || !p1 || !side1 || !tid2 || !p2 || !side2 || !v1 || !v2 || !shift || !stored1 || !stored2) return IM_E_ARG;
    for (int32_t q = 0; q < nq; q++) {
        if (tid1[q] < 0 || tid1[q] >= ctx->n_contigs || tid2[q] < 0 || tid2[q] >= ctx->n_contigs) {
            set_err(ctx, "im_cliptail_junction: query %d: contigs %d and %d, must be 0 .. %d", q, tid1[q], tid2[q], ctx->n_contigs - 1);
            return IM_E_ARG;
        }
        if (side1[q] > 1 || side2[q] > 1) { set_err(ctx, "im_cliptail_junction: query %d: sides %d and %d, must be 0 (right) or 1 (left)", q, (int)side1[q], (int)side2[q]); return IM_E_ARG; }
    }
    WsColumns C;                                                    // tid1, p1, tid2, p2, side1, side2, then the five answers
    rc = ws_columns(ctx, nq, 11, &C);
    const int32_t* h_in[4] = {tid1, p1, tid2, p2};
    for (int k = 0; k < 4 && !rc; k++) rc = C.down(k, h_in[k], 4);
    if (rc || (rc = C.down(4, side1, 1)) || (rc = C.down(5, side2, 1))) return rc;
    im::TailJunctionArgs A;
    A.nq = nq; A.max_shift = max_shift; A.tid1 = C.at<int32_t>(0); A.p1 = C.at<int32_t>(1); A.tid2 = C.at<int32_t>(2); A.p2 = C.at<int32_t>(3);
    A.side1 = C.at<uint8_t>(4); A.side2 = C.at<uint8_t>(5); A.ref = ref_dev(ctx); A.tab = ctx->tail;
    A.v1 = C.at<uint32_t>(6); A.v2 = C.at<uint32_t>(7); A.shift = C.at<int32_t>(8); A.stored1 = C.at<uint32_t>(9); A.stored2 = C.at<uint32_t>(10);
    HIP_TRY(ctx, im::launch_cliptail_junction(A, ctx->stream));
    return keyed_answers(ctx, ctx->tail, C, 6, {{v1, 4}, {v2, 4}, {shift, 4}, {stored1, 4}, {stored2, 4}});
}

int im_support_batch(im_ctx* ctx, int32_t n, const uint8_t* targets, const int64_t* t_off,
                     const uint8_t* queries, const int64_t* q_off, int32_t* out)
{
    if (!ctx || n < 0) return IM_E_ARG;
    if (n == 0) return IM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t tb = up256((size_t)t_off[n] + 16), qb = up256((size_t)q_off[n] + 16);
    const size_t ob = up256(sizeof(int64_t) * ((size_t)n + 1)), rb = up256(sizeof(int32_t) * 4 * (size_t)n);
    int64_t max_t = 0, max_q = 0;                                // max_t sizes the kernel's LDS; beyond the LDS form's bounds: the second launch
    for (int32_t i = 0; i < n; i++) {
        const int64_t l = t_off[i + 1] - t_off[i], q = q_off[i + 1] - q_off[i];
        if (l > max_t) max_t = l;
        if (q > max_q) max_q = q;
    }
    int32_t big_grid = 0;
    const size_t bigb = up256(im::support_big_scratch_bytes(max_t, max_q, n, &big_grid));
    int rc = ensure_ws(ctx, tb + qb + 2 * ob + rb + bigb);
    if (rc) return rc;
    char* w = static_cast<char*>(ctx->ws);
    uint8_t* d_t = (uint8_t*)w; w += tb;
    uint8_t* d_q = (uint8_t*)w; w += qb;
    int64_t* d_to = (int64_t*)w; w += ob;
    int64_t* d_qo = (int64_t*)w; w += ob;
    int32_t* d_out = (int32_t*)w; w += rb;
    void* d_big = (void*)w;
    HIP_TRY(ctx, hipMemcpyAsync(d_t, targets, (size_t)t_off[n], hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_q, queries, (size_t)q_off[n], hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_to, t_off, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_qo, q_off, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, im::launch_support(n, d_t, d_to, d_q, d_qo, d_out, max_t, max_q, d_big, big_grid, ctx->n_cu, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out, d_out, sizeof(int32_t) * 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int32_t i = 0; i < n; i++)
        if (out[4 * i + 3] == IM_ST_UNSUPPORTED) { set_err(ctx, "support task %d: target or query longer than the kernel holds", i); return IM_E_UNSUPPORTED; }
    return IM_OK;
}

int im_support_count(im_ctx* ctx, int32_t n_variants, const im_known_variant* variants, const uint8_t* alts, int64_t alt_bytes,
                     int32_t n_tasks, const im_count_task* tasks, const uint8_t* queries, int64_t query_bytes, int32_t* counts)
{
    if (!ctx || n_variants < 0 || n_tasks < 0 || alt_bytes < 0 || query_bytes < 0) return IM_E_ARG;
    if (n_variants == 0) { if (n_tasks > 0) { set_err(ctx, "im_support_count: tasks without variants"); return IM_E_ARG; } return IM_OK; }
    if (!variants || !counts || (n_tasks > 0 && !tasks) || (alt_bytes > 0 && !alts) || (query_bytes > 0 && !queries)) return IM_E_ARG;
    if (!ctx->ref_ascii) { set_err(ctx, "im_set_reference has not been called"); return IM_E_ARG; }
    if (alt_bytes > 0x7fffffffLL || query_bytes > 0x7fffffffLL) { set_err(ctx, "im_support_count: more than 2^31 bytes in one call"); return IM_E_ARG; }
    memset(counts, 0, sizeof(int32_t) * 3 * (size_t)n_variants);
    if (n_tasks == 0) return IM_OK;
    // every index the kernels follow is checked here, once
    for (int32_t v = 0; v < n_variants; v++) {
        const im_known_variant& k = variants[v];
        if (k.tid < 0 || k.tid >= ctx->n_contigs || k.start < 0 || k.stop < 0 || (k.type != IM_CLS_DELETION && k.type != IM_CLS_INSERTION) ||
            k.alt_off < 0 || k.alt_len < 0 || (int64_t)k.alt_off + k.alt_len > alt_bytes) {
            set_err(ctx, "im_support_count: variant %d is not a variant of this reference", v); return IM_E_ARG;
        }
    }
    std::vector<int32_t> big_idx;
    std::vector<int64_t> big_toff(1, 0);
    int64_t max_short = 0, max_big_t = 0, max_big_q = 0;
    for (int32_t i = 0; i < n_tasks; i++) {
        const im_count_task& t = tasks[i];
        if (t.variant < 0 || t.variant >= n_variants) { set_err(ctx, "im_support_count: task %d names variant %d of %d", i, t.variant, n_variants); return IM_E_ARG; }
        if (t.flags & IM_SC_DIRECT) continue;
        const im_known_variant& k = variants[t.variant];
        if (t.rstart < 0 || t.rstop < t.rstart || t.rstop > ctx->h_len[k.tid] || t.q_off < 0 || t.q_len < 0 || (int64_t)t.q_off + t.q_len > query_bytes) {
            set_err(ctx, "im_support_count: task %d reaches outside its contig or the query bytes", i); return IM_E_ARG;
        }
        if (t.q_len > im::support_count_max_query()) { set_err(ctx, "support task %d: query longer than the kernel holds", i); return IM_E_UNSUPPORTED; }
        const int64_t w = im::support_count_window(k, t.rstart, t.rstop);
        if (!im::support_count_is_big(w, t.q_len)) { if (w > max_short) max_short = w; continue; }
        big_idx.push_back(i);
        big_toff.push_back(big_toff.back() + w);
        if (w > max_big_t) max_big_t = w;
        if (t.q_len > max_big_q) max_big_q = t.q_len;
    }
    const int32_t n_big = (int32_t)big_idx.size();
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t big_grid = 0;
    const size_t rowb = n_big ? up256(im::support_big_scratch_bytes(max_big_t, max_big_q, n_big, &big_grid)) : 0;
    const size_t vb = up256(sizeof(im_known_variant) * (size_t)n_variants), ab = up256((size_t)alt_bytes + 16);
    const size_t kb = up256(sizeof(im_count_task) * (size_t)n_tasks), qb = up256((size_t)query_bytes + 16);
    const size_t cb = up256(sizeof(int32_t) * 3 * (size_t)n_variants);
    const size_t bib = up256(sizeof(int32_t) * (size_t)(n_big + 1)), bob = up256(sizeof(int64_t) * (size_t)(n_big + 1));
    const size_t bwb = up256((size_t)big_toff.back() + 16);
    int rc = ensure_ws(ctx, vb + ab + kb + qb + cb + bib + bob + bwb + rowb);
    if (rc) return rc;
    char* w = static_cast<char*>(ctx->ws);
    im_known_variant* d_v = (im_known_variant*)w; w += vb;
    uint8_t* d_a = (uint8_t*)w; w += ab;
    im_count_task* d_k = (im_count_task*)w; w += kb;
    uint8_t* d_q = (uint8_t*)w; w += qb;
    int32_t* d_c = (int32_t*)w; w += cb;
    int32_t* d_bi = (int32_t*)w; w += bib;
    int64_t* d_bo = (int64_t*)w; w += bob;
    uint8_t* d_bw = (uint8_t*)w; w += bwb;
    void* d_rows = (void*)w;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(d_v, variants, sizeof(im_known_variant) * (size_t)n_variants, hipMemcpyHostToDevice, st));
    if (alt_bytes > 0) HIP_TRY(ctx, hipMemcpyAsync(d_a, alts, (size_t)alt_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_k, tasks, sizeof(im_count_task) * (size_t)n_tasks, hipMemcpyHostToDevice, st));
    if (query_bytes > 0) HIP_TRY(ctx, hipMemcpyAsync(d_q, queries, (size_t)query_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(d_c, 0, sizeof(int32_t) * 3 * (size_t)n_variants, st));
    if (n_big > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(d_bi, big_idx.data(), sizeof(int32_t) * (size_t)n_big, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_bo, big_toff.data(), sizeof(int64_t) * (size_t)(n_big + 1), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(ctx, im::launch_support_count(n_tasks, d_k, d_v, d_a, ref_dev(ctx), d_q, d_c, max_short, n_big, d_bi, d_bo, d_bw, max_big_t, d_rows, big_grid,
                                          &ctx->support_count_attr, st));
    HIP_TRY(ctx, hipMemcpyAsync(counts, d_c, sizeof(int32_t) * 3 * (size_t)n_variants, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));      // the one synchronisation: big_idx / big_toff are read by then too
    return IM_OK;
}

int im_cluster_sr(im_ctx* ctx, int32_t n, const int32_t* cls, const int32_t* b1, const int32_t* b2,
                  int32_t marker, int32_t tie_desc,
                  int32_t* order, int32_t* cl_first, int32_t* cl_count, uint8_t* used, int32_t* n_clusters)
{
    if (!ctx || !n_clusters) return IM_E_ARG;
    if (n < 0) { set_err(ctx, "negative evidence count"); return IM_E_ARG; }
    *n_clusters = 0;
    if (n == 0) return IM_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // one flush (id 1) over slots [0, n), then the group-by of what it consumed.  Workspace and pinned staging share one
    // layout for the arrays that travel: cls, b1, b2 up in one copy; order, first, count, consumed and counts down in one.
    const size_t a32 = up256(sizeof(int32_t) * (size_t)n);
    const size_t up_bytes = 3 * a32, down_bytes = 4 * a32 + 256;
    const size_t gb_bytes = im::groupby_scratch_bytes(n);
    int rc = ensure_ws(ctx, up_bytes + down_bytes + up256(16 * (size_t)n) + 256 + gb_bytes);
    if (!rc) rc = ensure_pin(ctx, up_bytes + down_bytes);
    if (rc) return rc;
    char* w = static_cast<char*>(ctx->ws);
    char* h = static_cast<char*>(ctx->pin);
    auto arr = [&](char* base, int k) { return (int32_t*)(base + (size_t)k * a32); };
    int32_t *d_cls = arr(w, 0), *d_b1 = arr(w, 1), *d_b2 = arr(w, 2);
    char* d_down = w + up_bytes;
    int32_t *d_order = arr(d_down, 0), *d_first = arr(d_down, 1), *d_count = arr(d_down, 2), *d_consumed = arr(d_down, 3);
    int32_t* d_counts = arr(d_down, 4);
    int32_t* d_key = (int32_t*)(d_down + down_bytes);
    uint64_t* d_cut = (uint64_t*)(d_down + down_bytes + up256(16 * (size_t)n));
    void* d_gb = (char*)d_cut + 256;
    memcpy(arr(h, 0), cls, sizeof(int32_t) * (size_t)n);
    memcpy(arr(h, 1), b1, sizeof(int32_t) * (size_t)n);
    memcpy(arr(h, 2), b2, sizeof(int32_t) * (size_t)n);
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipMemcpyAsync(w, h, up_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemsetAsync(d_consumed, 0, sizeof(int32_t) * (size_t)n, st));
    HIP_TRY(ctx, hipMemsetAsync(d_cut, 0xFF, sizeof(uint64_t), st));
    HIP_TRY(ctx, im::launch_flush_cut(d_cls, d_b1, d_b2, d_consumed, 0, n, 0, 0, marker, 1, d_cut, nullptr, nullptr, 0, st));
    HIP_TRY(ctx, im::launch_groupby_init(n, d_gb, st));
    HIP_TRY(ctx, im::launch_groupby(n, n, nullptr, d_cls, d_b1, d_b2, d_consumed, tie_desc, d_order, d_key, d_first, d_count,
                                    d_counts, d_gb, st));
    HIP_TRY(ctx, hipMemcpyAsync(h + up_bytes, d_down, down_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    char* h_down = h + up_bytes;
    const int32_t *h_order = arr(h_down, 0), *h_first = arr(h_down, 1), *h_count = arr(h_down, 2), *h_consumed = arr(h_down, 3);
    const int32_t ncl = arr(h_down, 4)[0];
    // The clusters come back in table order.  Their keys are the host's own (b1, b2, cls) of a member: clusters ascending in
    // (b1, b2) (class is a function of (b1, b2), so the tie-break never decides), order[] rebuilt to match.
    struct Cl { uint64_t b12; int32_t cls, c; };
    std::vector<Cl> by(ncl);
    for (int32_t c = 0; c < ncl; c++) {
        const int32_t r = h_order[h_first[c]];
        by[c] = Cl{(uint64_t)((uint32_t)b1[r] ^ 0x80000000u) << 32 | ((uint32_t)b2[r] ^ 0x80000000u), cls[r], c};
    }
    std::sort(by.begin(), by.end(), [](const Cl& x, const Cl& y) { return x.b12 != y.b12 ? x.b12 < y.b12 : x.cls < y.cls; });
    int32_t pos = 0;
    for (int32_t k = 0; k < ncl; k++) {
        const int32_t c = by[k].c;
        cl_first[k] = pos; cl_count[k] = h_count[c];
        memcpy(order + pos, h_order + h_first[c], sizeof(int32_t) * (size_t)h_count[c]);
        pos += h_count[c];
    }
    for (int32_t i = 0; i < n; i++) used[i] = h_consumed[i] != 0;
    *n_clusters = ncl;
    return IM_OK;
}

struct im_timer { im_ctx* ctx; hipEvent_t a, b; };

int im_dev_alloc(im_ctx* ctx, size_t bytes, void** out)
{
    if (!ctx || !out) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMalloc(out, bytes ? bytes : 1));
    return IM_OK;
}
int im_dev_free(im_ctx* ctx, void* p)
{
    if (!ctx) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    { std::lock_guard<std::mutex> lk(ctx->gb_mu); ctx->gb_layout.erase(p); ctx->fg_layout.erase(p); }     // a group-by scratch: its address may come back as something else
    HIP_TRY(ctx, hipFree(p));
    return IM_OK;
}
int im_dev_memset(im_ctx* ctx, void* dst_dev, int byte, size_t bytes, void* stream)
{
    if (!ctx) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(dst_dev, byte, bytes, (hipStream_t)stream));
    return IM_OK;
}
int im_host_alloc(im_ctx* ctx, size_t bytes, void** out)
{
    if (!ctx || !out) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return IM_OK;
}
int im_host_free(im_ctx* ctx, void* p)
{
    if (!ctx) return IM_E_ARG;
    HIP_TRY(ctx, hipHostFree(p));
    return IM_OK;
}
int im_dev_upload_async(im_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes, void* stream)
{
    if (!ctx) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (bytes) HIP_TRY(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return IM_OK;
}
int im_dev_download_async(im_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes, void* stream)
{
    if (!ctx) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (bytes) HIP_TRY(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return IM_OK;
}
int im_dev_copy_async(im_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes, void* stream)
{
    if (!ctx) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (bytes) HIP_TRY(ctx, hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return IM_OK;
}
int im_dev_upload(im_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes)
{
    if (!ctx) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(dst_dev, src_host, bytes, hipMemcpyHostToDevice));
    return IM_OK;
}
int im_dev_download(im_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes)
{
    if (!ctx) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpy(dst_host, src_dev, bytes, hipMemcpyDeviceToHost));
    return IM_OK;
}
void* im_ctx_stream(im_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
int im_ctx_device(im_ctx* ctx) { return ctx ? ctx->device : -1; }
int im_stream_sync(im_ctx* ctx, void* stream)
{
    if (!ctx) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    return IM_OK;
}
int im_timer_create(im_ctx* ctx, im_timer** out)
{
    if (!ctx || !out) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    im_timer* t = new im_timer();
    t->ctx = ctx;
    hipError_t e = hipEventCreate(&t->a);
    if (e == hipSuccess) e = hipEventCreate(&t->b);
    if (e != hipSuccess) { set_err(ctx, "hipEventCreate: %s", hipGetErrorString(e)); delete t; return IM_E_HIP; }
    *out = t;
    return IM_OK;
}
void im_timer_destroy(im_timer* t)
{
    if (!t) return;
    (void)hipEventDestroy(t->a); (void)hipEventDestroy(t->b);
    delete t;
}
int im_timer_start(im_timer* t, void* stream)
{
    if (!t) return IM_E_ARG;
    HIP_TRY(t->ctx, hipEventRecord(t->a, (hipStream_t)stream));
    return IM_OK;
}
int im_timer_stop(im_timer* t, void* stream)
{
    if (!t) return IM_E_ARG;
    HIP_TRY(t->ctx, hipEventRecord(t->b, (hipStream_t)stream));
    return IM_OK;
}
int im_timer_elapsed_ms(im_timer* t, float* ms)
{
    if (!t || !ms) return IM_E_ARG;
    HIP_TRY(t->ctx, hipEventSynchronize(t->b));
    HIP_TRY(t->ctx, hipEventElapsedTime(ms, t->a, t->b));
    return IM_OK;
}

// ---- extra streams and events: overlap of one flush's clustering with the next flush's realign ------
struct im_event { im_ctx* ctx; hipEvent_t e; };

int im_stream_create(im_ctx* ctx, void** out)
{
    if (!ctx || !out) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // highest priority: the work put here is a handful of small kernels that must find wave slots while a
    // chip-filling realign launch of the context's own stream is in flight
    int lo = 0, hi = 0;
    HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));
    hipStream_t st = nullptr;
    HIP_TRY(ctx, hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi));
    *out = (void*)st;
    return IM_OK;
}
int im_stream_destroy(im_ctx* ctx, void* stream)
{
    if (!ctx || !stream) return IM_E_ARG;
    HIP_TRY(ctx, hipStreamDestroy((hipStream_t)stream));
    return IM_OK;
}
int im_event_create(im_ctx* ctx, im_event** out)
{
    if (!ctx || !out) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipEvent_t e = nullptr;
    HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    im_event* r = new im_event();
    r->ctx = ctx; r->e = e;
    *out = r;
    return IM_OK;
}
void im_event_destroy(im_event* ev)
{
    if (!ev) return;
    (void)hipEventDestroy(ev->e);
    delete ev;
}
int im_event_record(im_event* ev, void* stream)
{
    if (!ev) return IM_E_ARG;
    HIP_TRY(ev->ctx, hipEventRecord(ev->e, (hipStream_t)stream));
    return IM_OK;
}
// record on `from`, make `to` wait: one call for the usual producer -> consumer hand-over
int im_stream_follow(im_event* ev, void* from, void* to)
{
    if (!ev) return IM_E_ARG;
    HIP_TRY(ev->ctx, hipEventRecord(ev->e, (hipStream_t)from));
    HIP_TRY(ev->ctx, hipStreamWaitEvent((hipStream_t)to, ev->e, 0));
    return IM_OK;
}
int im_event_sync(im_event* ev)
{
    if (!ev) return IM_E_ARG;
    HIP_TRY(ev->ctx, hipEventSynchronize(ev->e));
    return IM_OK;
}
int im_stream_wait_event(im_ctx* ctx, void* stream, im_event* ev)
{
    if (!ctx || !ev) return IM_E_ARG;
    HIP_TRY(ctx, hipStreamWaitEvent((hipStream_t)stream, ev->e, 0));
    return IM_OK;
}

// ---- launch graphs -----------------------------------------------------------------
// A flush is a fixed sequence of small dependent launches (realign, then the cluster kernels); captured
// once into a HIP graph it is replayed with one host call and without per-launch submission gaps.
struct im_graph { im_ctx* ctx; hipGraph_t g; hipGraphExec_t x; };

int im_capture_begin(im_ctx* ctx, void* stream)
{
    if (!ctx) return IM_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
    return IM_OK;
}
int im_capture_end(im_ctx* ctx, void* stream, im_graph** out)
{
    if (!ctx || !out) return IM_E_ARG;
    hipGraph_t g = nullptr;
    HIP_TRY(ctx, hipStreamEndCapture((hipStream_t)stream, &g));
    hipGraphExec_t x = nullptr;
    hipError_t e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    if (e != hipSuccess) { (void)hipGraphDestroy(g); set_err(ctx, "hipGraphInstantiate: %s", hipGetErrorString(e)); return IM_E_HIP; }
    im_graph* r = new im_graph();
    r->ctx = ctx; r->g = g; r->x = x;
    *out = r;
    return IM_OK;
}
int im_graph_launch(im_graph* g, void* stream)
{
    if (!g) return IM_E_ARG;
    HIP_TRY(g->ctx, hipGraphLaunch(g->x, (hipStream_t)stream));
    return IM_OK;
}
void im_graph_destroy(im_graph* g)
{
    if (!g) return;
    (void)hipGraphExecDestroy(g->x); (void)hipGraphDestroy(g->g);
    delete g;
}

}  // extern "C"
