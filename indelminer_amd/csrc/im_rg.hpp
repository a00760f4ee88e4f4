// im_rg.hpp -- what more than one kernel needs of a delivered BAM record: the view of its core and variable part, the sliding
// window over its aux area, the walk to its RG / MQ tags and the read-group -> range[1] table look-up.  Device code only; used by
// im_triage.hip (the classify kernel) and im_span.hip (the concordant-pair scatter).  Every includer gets its own copy (unnamed
// namespace), as with the helpers of im_wave.hpp.

#pragma once

#include "im_device.hpp"

namespace im {
namespace {

__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }

struct RecView {
    const uint8_t* p;       // record start (the 32-byte core)
    uint32_t len;           // bytes of the record
    int32_t tid, pos, mtid, mpos, isize, l_seq;
    uint32_t l_qname, mapq, n_cigar, flag;
    uint32_t o_cigar, o_seq, o_aux;
    uint32_t cig[4];        // the first four CIGAR words, loaded together with the aux window
    bool ok;
};

constexpr int kAuxWin = 24;     // bytes of the aux area a lane holds in LDS at a time: the tag walk slides the window along (aux_slide); more LDS
                                // would cost the kernel its sixth workgroup per CU

__device__ __forceinline__ RecView view_record(const uint8_t* raw, uint32_t off, uint32_t end)
{
    RecView r;
    r.p = raw + off; r.len = end - off; r.ok = false;
    r.tid = r.pos = r.mtid = r.mpos = r.isize = r.l_seq = 0;
    r.l_qname = r.mapq = r.n_cigar = r.flag = 0; r.o_cigar = r.o_seq = r.o_aux = 0;
    r.cig[0] = r.cig[1] = r.cig[2] = r.cig[3] = 0;
    if (end < off || r.len < 32u) return r;
    const uint32_t* c = reinterpret_cast<const uint32_t*>(r.p);     // 4-byte aligned by contract
    r.tid = (int32_t)c[0]; r.pos = (int32_t)c[1];
    const uint32_t w2 = c[2], w3 = c[3];
    r.l_qname = w2 & 255u; r.mapq = (w2 >> 8) & 255u;
    r.n_cigar = w3 & 0xFFFFu; r.flag = w3 >> 16;
    r.l_seq = (int32_t)c[4]; r.mtid = (int32_t)c[5]; r.mpos = (int32_t)c[6]; r.isize = (int32_t)c[7];
    if (r.l_seq < 0) return r;
    r.o_cigar = 32u + r.l_qname;
    r.o_seq = r.o_cigar + 4u * r.n_cigar;
    // a record delivered without its base qualities says so in its bin field (include/indelminer_amd.h, im_dev_records)
    const bool no_qual = (w2 >> 16) == 0xFFFFu;
    const uint64_t o_aux = (uint64_t)r.o_seq + (((uint64_t)r.l_seq + 1u) >> 1) + (no_qual ? 0ull : (uint64_t)r.l_seq);
    if (o_aux > r.len) return r;
    r.o_aux = (uint32_t)o_aux;
    r.ok = true;
    return r;
}

__device__ __forceinline__ int aux_size(uint32_t t)
{
    // selects, not a switch: the tag walk calls it in straight-line code
    return (t == 'A' || t == 'c' || t == 'C') ? 1 : (t == 's' || t == 'S') ? 2 : (t == 'i' || t == 'I' || t == 'f') ? 4 : t == 'd' ? 8 : 0;
}

// a byte of the record at offset o: the lane's aux window (LDS) when it covers o, memory otherwise
struct AuxWin { uint32_t* lds; uint32_t o0; };
__device__ __forceinline__ uint32_t rec_byte(const RecView& r, const AuxWin& w, uint32_t o)
{
    const uint32_t d = o - w.o0;
    return d < (uint32_t)kAuxWin ? reinterpret_cast<const uint8_t*>(w.lds)[d] : r.p[o];
}
// The window moved to offset o: six dword loads by the lane that needs them, issued together and waited for once -- the values
// are held in registers until all six are under way, then written (a load and its LDS write per dword made six round trips one
// after the other).  What an aligner writes in front of RG and MQ (NM MD AS XS MC ...: 30-100 bytes) used to be walked through
// memory byte by byte behind the first 24 -- every byte a 64-line gather: records with such fields took classify from 25 to 77 us
// per 300 000 (profiles/r04_m_*).  Reads past the record stay inside the chunk buffer (>= 64 spare bytes behind the last record):
// o < r.len wherever the window is moved, so the last byte read is at most 23 behind the record's end.
__device__ __forceinline__ void aux_slide(const RecView& r, AuxWin& w, uint32_t o)
{
    w.o0 = o;
    uint32_t v[kAuxWin / 4];
#pragma unroll
    for (int k = 0; k < kAuxWin / 4; k++) v[k] = ld_u32(r.p + o + 4u * k);
#pragma unroll
    for (int k = 0; k < kAuxWin / 4; k++) w.lds[k] = v[k];
}
// the byte at o for a walk that only moves forward: the window follows
__device__ __forceinline__ uint32_t walk_byte(const RecView& r, AuxWin& w, uint32_t o)
{
    if (o - w.o0 >= (uint32_t)kAuxWin) aux_slide(r, w, o);
    return reinterpret_cast<const uint8_t*>(w.lds)[o - w.o0];
}
// [o, o + need) inside the window (need <= kAuxWin)
__device__ __forceinline__ bool aux_covers(const AuxWin& w, uint32_t o, uint32_t need)
{
    return o >= w.o0 && o + need <= w.o0 + (uint32_t)kAuxWin;
}
__device__ __forceinline__ void aux_cover(const RecView& r, AuxWin& w, uint32_t o, uint32_t need)
{
    if (!aux_covers(w, o, need)) aux_slide(r, w, o);
}
// a byte the window is known to cover; a lane that is not `on` reads the window's first byte and makes nothing of it
__device__ __forceinline__ uint32_t win_byte(const AuxWin& w, uint32_t o, bool on)
{
    return reinterpret_cast<const uint8_t*>(w.lds)[on ? o - w.o0 : 0u];
}

// bam_aux_get for RG and MQ in one walk (bam_aux.c:27-54): offsets of the TYPE byte of the first
// occurrence, 0 = absent.  The walk stops where samtools' would (unknown type, truncated B array).
// The loops are the WAVE's: a pass per field while any lane of the caller still walks, the lanes that are done (or that do not
// walk at all: `walk` false) predicated, and what few fields need -- a window that has to move, a string, a B array -- behind a
// test on the whole wave.  A wave of records with fixed-size fields inside the first window runs no lane-divergent region.
__device__ __forceinline__ void find_rg_mq(const RecView& r, AuxWin& w, uint32_t& o_rg, uint32_t& o_mq, bool walk = true)
{
    o_rg = 0; o_mq = 0;
    uint32_t s = r.o_aux;
    const uint32_t end = r.len;
    bool on = walk && s + 4u <= end;     // a tail of < 4 bytes is alignment padding (include/indelminer_amd.h, im_dev_records)
    while (__ballot(on) != 0ull) {
        // tag, type and what a B array's header takes
        const bool move = on && !aux_covers(w, s, 8u);
        if (__ballot(move) != 0ull) { if (move) aux_slide(r, w, s); }
        const uint32_t t0 = win_byte(w, s, on), t1 = win_byte(w, s + 1u, on), type = win_byte(w, s + 2u, on);
        if (on && t0 == 'R' && t1 == 'G' && !o_rg) o_rg = s + 2u;
        if (on && t0 == 'M' && t1 == 'Q' && !o_mq) o_mq = s + 2u;
        on = on && !(o_rg && o_mq);
        s += 3u;
        const bool str = on && (type == 'Z' || type == 'H'), arr = on && type == 'B';
        const uint32_t sz = (uint32_t)aux_size(type);
        if (on && !str && !arr) { on = sz != 0u; s += sz; }
        if (__ballot(str) != 0ull) {
            // while (s < end && byte(s)) s++; s++;
            bool go = str;
            for (;;) {
                go = go && s < end;
                const bool mv = go && s - w.o0 >= (uint32_t)kAuxWin;
                if (__ballot(mv) != 0ull) { if (mv) aux_slide(r, w, s); }
                go = go && win_byte(w, s, go) != 0u;
                if (__ballot(go) == 0ull) break;
                s += go ? 1u : 0u;
            }
            s += str ? 1u : 0u;
        }
        if (__ballot(arr) != 0ull) {
            // the header's five bytes lie in the window: it covers eight bytes from the tag on
            const bool hdr = arr && s + 5u <= end;
            const uint32_t esz = (uint32_t)aux_size(win_byte(w, s, hdr));
            const uint32_t cnt = win_byte(w, s + 1u, hdr) | (win_byte(w, s + 2u, hdr) << 8) | (win_byte(w, s + 3u, hdr) << 16) | (win_byte(w, s + 4u, hdr) << 24);
            const uint64_t ns = (uint64_t)s + 5u + (uint64_t)esz * cnt;        // 64 bits: count * size can pass 2^32
            const bool fits = hdr && ns <= end;
            if (arr) { on = fits; s = fits ? (uint32_t)ns : s; }
        }
        on = on && s + 4u <= end;
    }
}

// bam_aux_get for ONE tag (t0, t1), by find_rg_mq's walk rules and in its shape -- the loops are the wave's, the lanes that do not
// walk (`walk` false) or are done predicated: the offset of the TYPE byte of the first occurrence (0 = absent) and, in *type, that
// byte.  A lane that walks moves its window itself (o0 = 0 covers no aux byte: an aux area starts behind the 32-byte core), so the
// caller loads nothing for the lanes that do not walk.  Used by the split-link scatter (im_links.hip); the classify kernel does not
// call it.
__device__ __forceinline__ uint32_t find_tag(const RecView& r, AuxWin& w, uint32_t t0, uint32_t t1, bool walk, uint32_t* type_out)
{
    uint32_t found = 0;
    *type_out = 0;
    uint32_t s = r.o_aux;
    const uint32_t end = r.len;
    bool on = walk && s + 4u <= end;
    while (__ballot(on) != 0ull) {
        const bool move = on && !aux_covers(w, s, 8u);
        if (__ballot(move) != 0ull) { if (move) aux_slide(r, w, s); }
        const uint32_t b0 = win_byte(w, s, on), b1 = win_byte(w, s + 1u, on), type = win_byte(w, s + 2u, on);
        if (on && b0 == t0 && b1 == t1) { found = s + 2u; *type_out = type; on = false; }
        s += 3u;
        const bool str = on && (type == 'Z' || type == 'H'), arr = on && type == 'B';
        const uint32_t sz = (uint32_t)aux_size(type);
        if (on && !str && !arr) { on = sz != 0u; s += sz; }
        if (__ballot(str) != 0ull) {
            bool go = str;
            for (;;) {
                go = go && s < end;
                const bool mv = go && s - w.o0 >= (uint32_t)kAuxWin;
                if (__ballot(mv) != 0ull) { if (mv) aux_slide(r, w, s); }
                go = go && win_byte(w, s, go) != 0u;
                if (__ballot(go) == 0ull) break;
                s += go ? 1u : 0u;
            }
            s += str ? 1u : 0u;
        }
        if (__ballot(arr) != 0ull) {
            const bool hdr = arr && s + 5u <= end;
            const uint32_t esz = (uint32_t)aux_size(win_byte(w, s, hdr));
            const uint32_t cnt = win_byte(w, s + 1u, hdr) | (win_byte(w, s + 2u, hdr) << 8) | (win_byte(w, s + 3u, hdr) << 16) | (win_byte(w, s + 4u, hdr) << 24);
            const uint64_t ns = (uint64_t)s + 5u + (uint64_t)esz * cnt;
            const bool fits = hdr && ns <= end;
            if (arr) { on = fits; s = fits ? (uint32_t)ns : s; }
        }
        on = on && s + 4u <= end;
    }
    return found;
}

// The insert-length table as one blob (LDS copy when it is small, else the device original):
// [bin_start 17][name_off n][name_len n][range_max n][names]
struct RgView {
    const int32_t* bin_start; const int32_t* name_off; const int32_t* name_len; const int32_t* range_max; const uint8_t* names;
};
__device__ __forceinline__ RgView rg_view(const uint8_t* blob, int32_t n)
{
    RgView v;
    const int32_t* w = reinterpret_cast<const int32_t*>(blob);
    const int32_t m = n > 0 ? n : 1;
    v.bin_start = w; v.name_off = w + 20; v.name_len = w + 20 + m; v.range_max = w + 20 + 2 * m;
    v.names = blob + 4 * (20 + 3 * m);
    return v;
}

// must_find_hashtable(insertlengths, rgname, strlen(rgname)) (src/indelminer.c:374-376): DJB2 over the
// bytes back to front (src/hashfunc.c:23-30), 16 bins, the chain walked head to tail, strncmp prefix
// match, LAST hit wins (src/hashtable.c:62-81).  Returns false when the reference would exit.
template <typename NameAt>
__device__ __forceinline__ bool rg_lookup(const RgView& T, NameAt name_at, uint32_t len, int32_t& range_max)
{
    uint32_t h = 5381u;
    for (int i = (int)len - 1; i >= 0; i--) h += (h << 5) + (uint32_t)(int32_t)(int8_t)name_at((uint32_t)i);
    const uint32_t bin = h & 15u;
    bool hit = false;
    for (int32_t e = T.bin_start[bin]; e < T.bin_start[bin + 1]; e++) {
        const uint32_t el = (uint32_t)T.name_len[e];
        if (el < len) continue;                      // the stored name ends first: strncmp sees NUL != byte
        const uint8_t* en = T.names + T.name_off[e];
        bool same = true;
        for (uint32_t i = 0; i < len && same; i++) same = en[i] == name_at(i);
        if (same) { hit = true; range_max = T.range_max[e]; }
    }
    return hit;
}

// The range of the read group an RG tag names (o_rg: the tag's TYPE byte).  false where the reference would exit: a tag that
// bam_aux2Z refuses (strlen(NULL)), a name that is not in the table.
__device__ __forceinline__ bool rg_tag_range(const RecView& r, AuxWin& w, uint32_t o_rg, const RgView& T, int32_t& range_max)
{
    const uint32_t type = rec_byte(r, w, o_rg);
    bool ok = type == 'Z' || type == 'H';                                  // else bam_aux2Z returns NULL: strlen(NULL)
    if (ok) {
        // the name's length; a name that runs out of the window brings the window to the tag (names of up to 22 bytes then lie in it)
        uint32_t len = 0;
        while (o_rg + 1u + len < r.len) {
            const uint32_t o = o_rg + 1u + len;
            if (o - w.o0 >= (uint32_t)kAuxWin && w.o0 != o_rg) aux_slide(r, w, o_rg);
            if (!rec_byte(r, w, o)) break;
            len++;
        }
        const uint32_t o_name = o_rg + 1u;
        ok = rg_lookup(T, [&](uint32_t k) { return rec_byte(r, w, o_name + k); }, len, range_max);
    }
    return ok;
}

constexpr int kRgLds = 2048;        // an insert-length table up to this size is copied to LDS

}  // namespace
}  // namespace im
