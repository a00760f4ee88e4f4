/*
 * indelminer_amd.h -- C ABI of the MI355X (gfx950) split-read hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Each entry point names the reference interface it replaces (file:line under
 * ratan-lab/indelMINER).  The library is libindelminer_amd.so, built from
 * indelminer_amd/csrc/ with hipcc --offload-arch=gfx950.  There is NO CPU
 * fallback: every compute entry point needs a GPU and returns IM_E_NOGPU /
 * IM_E_HIP loudly without one.
 *
 * Two levels:
 *   im_realign_batch / im_cluster_sr      host buffers in, host buffers out
 *                                         (what the C host driver calls);
 *   im_dev_*                              same kernels on caller-owned device
 *                                         buffers and a caller-owned stream
 *                                         (bench.py, multi-GPU plumbing).
 */
#ifndef INDELMINER_AMD_H
#define INDELMINER_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IM_ABI_VERSION 3

/* ---- return codes ------------------------------------------------------ */
#define IM_OK             0
#define IM_E_ARG         -1     /* bad argument                                      */
#define IM_E_NOGPU       -2     /* no HIP device / wrong architecture                */
#define IM_E_HIP         -3     /* a HIP runtime call failed (see im_last_error)     */
#define IM_E_UNSUPPORTED -4     /* parameters outside what the kernels implement     */
#define IM_E_ABORT       -5     /* a read hit a condition on which the reference
                                   exits (forceassert, src/asserts.h:9-19)           */
#define IM_E_OVERFLOW    -6     /* a fixed bound (IM_MAX_OPS / IM_MAX_EV) exceeded   */

/* ---- per-read status (im_read_result.status) --------------------------- */
#define IM_ST_NONE        0     /* attempt_pe_alignment returned NULL                */
#define IM_ST_EVIDENCE    1     /* segment list + n_ev >= 1 evidence records valid   */
#define IM_ST_ABORT      -1     /* the reference would have exited on this read      */
#define IM_ST_OVERFLOW   -2     /* the read's result is beyond IM_MAX_OPS or IM_MAX_EV (the reference has neither bound).
                                 * The rule, with (n_ops, n_ev) what the reference's attempt_pe_alignment leaves for the read:
                                 *   n_ops <= IM_MAX_OPS and n_ev <= IM_MAX_EV   IM_ST_EVIDENCE, every field as the reference has it
                                 *                                                (a list of exactly 64 words, 4 indels: they fit)
                                 *   n_ops >  IM_MAX_OPS or  n_ev >  IM_MAX_EV   IM_ST_OVERFLOW
                                 * One case the rule leaves open: a final list that fits while the CIGAR of one of the two band
                                 * alignments it is cut from is beyond IM_MAX_OPS words -- IM_ST_OVERFLOW today.
                                 * An overflow record holds n_ev = n_ops = ref_start = 0 (like every status but IM_ST_EVIDENCE),
                                 * n_band and band[] as for a read that fitted (both band searches were done; band[1] is zero when the
                                 * FIRST alignment's CIGAR was the one too long, n_band = 1 then), nothing valid in ev[] and ops[], and
                                 * nothing outside its 512 bytes.  Its evidence slots (im_dev_batch.ev_cls/b1/b2): cls = -1, b1 = b2 = 0
                                 * in all IM_MAX_EV of them from im_dev_realign; untouched by im_dev_realign_keep (and
                                 * im_dev_realign_n with keep_slots = 1), like those of a read without realigned evidence.
                                 * im_realign_batch returns IM_E_OVERFLOW when a read of the batch overflowed (every record is
                                 * written, im_last_error names the first such read); im_dev_compact_results does not pack it.
                                 * Which kernel can meet which bound: a list grows by at most 2 words per ~12 read bases, so the
                                 * segment bound takes a read of some 450 bases or more -- the long-read kernel and the general
                                 * pass; numgaps == 0 leaves one indel per read, so the indel bound takes numgaps > 0 -- the band
                                 * kernel and the general pass.  tests/test_gpu_record_bounds.py holds all of this. */
#define IM_ST_UNSUPPORTED -3    /* a read beyond 255 bases when im_expect_read_length was not told of it; base_off not a multiple of 4 */

/* CIGAR op codes in packed words (len<<4|op): samtools bam.h + src/readaln.h:10-11 */
#define IM_OP_M  0
#define IM_OP_I  1
#define IM_OP_D  2
#define IM_OP_S  4
#define IM_OP_EQ 7
#define IM_OP_X  8

#define IM_MAX_READ  1020       /* longest read of the LAID-OUT realign kernels (numgaps == 0; 255 with numgaps > 0); longer
                                   reads -- the reference takes any, src/readaln.c:242-267 -- run in a general pass behind them,
                                   see im_expect_read_length */
#define IM_MAX_SW_TARGET 4095   /* longest annotate-mode window (reference span + variant) of im_support_batch's LDS form; longer
                                   windows and queries beyond IM_MAX_READ run in its second form */
#define IM_MAX_OPS   64         /* packed segment words per realigned read: 64 fit, 65 are IM_ST_OVERFLOW (see there) */
#define IM_MAX_EV    4          /* indel segments (= evidence) per realigned read: 4 fit, 5 are IM_ST_OVERFLOW         */

#define IM_CLS_INSERTION 0      /* varianttype, src/evidence.h:13-17                 */
#define IM_CLS_DELETION  1

typedef struct im_ctx im_ctx;
typedef struct im_comm im_comm;         /* an RCCL communicator (multi-GPU section below) */

/* The globals the reference path reads (src/alignment.c:3-9), set from the CLI
 * (src/indelminer.c:930-944): -k, -g, -s, -n. */
typedef struct im_params {
    uint32_t klength;           /* 2..15, default 6    */
    uint32_t numgaps;           /* default 0           */
    uint32_t maxdelsize;        /* default 1000        */
    uint32_t ethreshold;        /* default 10          */
} im_params;

/* One evidence record = one D/I segment of a realigned read
 * (new_evidence, src/evidence.c:4-34) plus the per-evidence reductions
 * print_variants / print_vcf_output take over aln1/aln3 (src/variant.c:217-290,704-775). */
typedef struct im_evidence {
    int32_t cls;                /* IM_CLS_*                                          */
    int32_t b1, b2;             /* segment [start,end) on the contig, 0-based        */
    int32_t seg;                /* index of the segment in ops[]                     */
    int32_t read_off;           /* read offset of the segment's first base           */
    int32_t lflank, rflank;     /* M/=/X/I bases left / right of the segment         */
    int32_t nd_print;           /* X+I+D bases in aln1+aln3 (DF=)                    */
    int32_t nd_filter;          /* nd_print + soft-clipped bases (-f filter)         */
} im_evidence;

/* One raw band alignment (attempt_band_alignment, src/alignment.c:343-391). */
typedef struct im_band_aln {
    int32_t r1, r2, q1, q2;     /* 0-based half-open contig / read coordinates       */
    int32_t low;                /* diagonal chosen by find_best_band                 */
    int32_t votes;              /* k-mer votes on that band                          */
    int32_t win_bytes;          /* reference window bytes scanned (roofline book-keeping) */
    int32_t piece_bytes;        /* read piece bytes                                  */
} im_band_aln;

/* What attempt_pe_alignment (src/alignment.c:764-799) leaves behind for one read. */
typedef struct im_read_result {
    int32_t status;             /* IM_ST_*                                           */
    int32_t ref_start;          /* contig coordinate of the first segment            */
    int32_t n_ops;              /* words valid in ops[]                              */
    int32_t n_ev;               /* records valid in ev[]                             */
    int32_t n_band;             /* band searches done (0, 1 or 2)                    */
    int32_t reserved[7];        /* pads the record to 512 bytes */
    im_band_aln band[2];
    im_evidence ev[IM_MAX_EV];  /* in segment order, left to right                   */
    uint32_t ops[IM_MAX_OPS];   /* final segment list, update_readsegs (src/readaln.c:348-458) */
} im_read_result;

/* A batch of candidate reads, struct-of-arrays.  Replaces the per-read
 * arguments of attempt_pe_alignment(sequences, tid, position, range, rln)
 * (src/alignment.h:21-25, call sites src/indelminer.c:411,486). */
typedef struct im_read_batch {
    int32_t        n;           /* reads                                             */
    const uint8_t* bases;       /* ASCII read bases, concatenated; already reverse-
                                   complemented where the caller decided so
                                   (src/indelminer.c:404-409,479-484)                */
    const int64_t* base_off;    /* n+1 offsets into bases                            */
    const int32_t* tid;         /* mate contig  (core.mtid), an index into the contigs
                                   of im_set_reference.  A read whose tid lies outside
                                   [0, n_contigs) touches no reference byte: its result
                                   is IM_ST_ABORT with n_ev = 0 (the call returns
                                   IM_E_ABORT), whatever its length and the parameters,
                                   and the other reads of the batch are not affected.
                                   The same holds for im_dev_batch.tid.              */
    const int32_t* anchor;      /* mate position (core.mpos)                         */
    const int32_t* range_max;   /* range[1] of the read group                        */
} im_read_batch;

/* ---- context ----------------------------------------------------------- */

/* Open HIP device `device` (must be gfx950).  One context per GPU. */
int  im_ctx_create(int device, im_ctx** out);
void im_ctx_destroy(im_ctx* ctx);
/* Last error text of this context (or of im_ctx_create when ctx == NULL). */
const char* im_last_error(const im_ctx* ctx);
int  im_abi_version(void);

/* Make the reference contigs resident in HBM.  seqs[i] is contig i exactly as
 * read_reference keeps it (upper-cased ASCII, src/shared.c:46-82); lens[i] its
 * length.  Replaces the `char** sequences` argument of attempt_pe_alignment. */
int im_set_reference(im_ctx* ctx, int32_t n_contigs,
                     const char* const* seqs, const int64_t* lens);

/* ---- seam 1: split-read realignment ------------------------------------ */

/* Realign every read of the batch: per read, the exact result of
 * attempt_pe_alignment (src/alignment.c:764-799).  out[] has batch->n entries.
 * Returns IM_OK, or IM_E_ABORT / IM_E_OVERFLOW / IM_E_UNSUPPORTED if any read
 * ended in the corresponding status (all results are still written). */
int im_realign_batch(im_ctx* ctx, const im_params* params,
                     const im_read_batch* batch, im_read_result* out);

/* ---- seam 2: split-read clustering -------------------------------------- */

/* The split-read part of process_evidence (src/indelminer.c:117-209 with the
 * SR rule of add_node, src/graph.c:122-127): evidence arrives as parallel
 * arrays in ARRIVAL order; it is sorted by (b1,b2), cut at the first
 * b2 >= marker, and grouped by identical (cls,b1,b2).  For identical (b1,b2)
 * every record has the same class by construction (insertions have b1 == b2,
 * deletions b2 > b1), so the groups are the reference's runs in sorted order.
 * cls is a split-read class (0 or 1).  One im_dev_flush_cut over [0, n) and
 * one im_dev_cluster_groupby; the host orders the clusters.
 *   order[n]     evidence indices, cluster after cluster, clusters ascending
 *                in (b1,b2); members ascending in arrival (tie_desc = 0, what
 *                glibc's stable qsort yields) or descending (tie_desc = 1, the
 *                order test_data/indelminer.expected.vcf was made with)
 *   cl_first/cl_count[n]  slice of order[] per cluster
 *   used[n]      1 for every evidence that became a graph node
 *   n_clusters   number of clusters
 */
int im_cluster_sr(im_ctx* ctx, int32_t n,
                  const int32_t* cls, const int32_t* b1, const int32_t* b2,
                  int32_t marker, int32_t tie_desc,
                  int32_t* order, int32_t* cl_first, int32_t* cl_count,
                  uint8_t* used, int32_t* n_clusters);

/* ---- seam 3: region depth (DP=) ------------------------------------------------- */

/* Replaces calculate_cov_params(bam_name, tid, start, stop) (src/shared.c:178-212), which the
 * reference calls once per printed variant and which re-opens the BAM, reloads the index and
 * pileups the region each time.  im_depth_build takes, once per contig, the M/=/X segments
 * (contig start, length) of every record samtools' pileup would count (not unmapped, secondary,
 * QC-fail or duplicate; bam_pileup.c:171-172) and leaves the per-position depth resident on the
 * device; im_depth_query returns, per query, the SUM of depths over [beg, end) -- the caller
 * divides by the length and floors (src/shared.c:205). */
int im_depth_build(im_ctx* ctx, int64_t contig_len, int32_t n_seg,
                   const int32_t* seg_start, const int32_t* seg_len);
int im_depth_query(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* sum_out);
/* the same, and per query the DEEPEST position of [beg - 1, end] (max_out, may be NULL): what im_depth_query_max_tid answers on the
 * genome-wide array (same definition, same edges), here on what im_depth_build left.  The record-at-a-time path of the host driver
 * decides with it, like the pipelined path, whether samtools' pileup cap may have applied to a DP=. */
int im_depth_query_max(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* sum_out, uint32_t* max_out);
/* Seam 3's order statistic (no reference counterpart: calculate_cov_params only ever sums, src/shared.c:178-212), over what
 * im_depth_build left.  Per query [beg, end), clipped to [0, contig_len), the LOWER MEDIAN of the depths of its n positions: the
 * smallest d such that at least (n + 1) / 2 of them have depth <= d.  A position with depth >= 4095 counts as 4095 -- the
 * median saturates there.  A query that is empty after the clip (beg >= end included) answers 0xFFFFFFFF.  Exact for an
 * interval of any length; one launch and one wait per call.  IM_E_ARG before im_depth_build, like im_depth_query. */
int im_depth_median(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* med_out);

/* ---- seam 4: annotate mode, "is this known indel supported by this read?" ------- */

/* Replaces the Smith-Waterman inside realign_with_indel (src/variant.c:1246-1424), called from
 * check_for_indel (1427-1556) for every read overlapping a known split-read variant that the
 * discovery pass did not re-find.  Task i aligns query i (the aligned part of a read,
 * read[qstart,qstop)) against target i (the reference window with the variant applied, built by
 * the caller exactly as 1260-1272 do) and returns the three counts check_for_indel compares with
 * the read's existing alignment (1549-1553): substitutions, inserted+deleted bases, aligned bases.
 * targets/queries: concatenated bytes with n+1 offsets.  out: n x 4 int32 {subs, indels, aligned,
 * status (IM_ST_EVIDENCE = valid; IM_ST_UNSUPPORTED only for a query beyond 2^20 bases)}.  Targets and queries of any
 * length: within IM_MAX_SW_TARGET / IM_MAX_READ the task runs with its boundary row in LDS, beyond in device memory. */
int im_support_batch(im_ctx* ctx, int32_t n,
                     const uint8_t* targets, const int64_t* t_off,
                     const uint8_t* queries, const int64_t* q_off, int32_t* out);

/* ---- seam 4, counting form: "how many reads support this known indel?" (-A) ------ */

/* check_for_indel's rule (src/variant.c:1427-1573) for EVERY read that overlaps a known variant, not up to the first that
 * passes (is_indel_supported, 1561-1573, stops there): the read counts for and against each known indel of an annotate run.
 * No reference counterpart for the counts; the per-read rule is the reference's.
 * One call takes the tasks of many variants.  A task names its variant and the stretch [rstart, rstop) of the contig its read
 * covers, widened by the indel's size and clipped to the contig by the caller (1259-1263); the kernel reads the window through
 * the splice from the resident reference (im_set_reference) and the variant's ALT bytes -- the caller builds no window:
 *     deletion   ref[rstart, start) + ref[stop-1, rstop)          insertion   ref[rstart, start) + ALT[1..] + ref[start, rstop)
 * (raw bytes: the score compares upper-cased bytes, the substitution count raw ones), runs im_support_batch's Smith-Waterman of
 * queries[q_off, q_off + q_len) against it and applies the verdict subs <= own_subs, indels <= own_indels, aligned >= own_aligned.
 * IM_SC_DIRECT: the read's CIGAR carries the indel itself, it supports without an alignment.  Per variant the call returns
 *     counts[3v]     N_all  supporting tasks
 *     counts[3v+1]   AS     ... that have IM_SC_MAPQ_OK
 *     counts[3v+2]   DC     ... that have IM_SC_MAPQ_OK and IM_SC_SPANS (reads seam 5's array has counted for the reference)
 * Integer adds: the result does not depend on the order of the tasks.  Windows beyond IM_MAX_SW_TARGET and queries beyond
 * IM_MAX_READ (up to 2^20 bases) are counted too, by a second launch.  Stream-ordered on the context's stream, one
 * synchronisation when the counts come back. */
#define IM_SC_DIRECT   1
#define IM_SC_MAPQ_OK  2
#define IM_SC_SPANS    4
typedef struct {
    int32_t tid;                /* contig of im_set_reference                          */
    int32_t start, stop;        /* POS and END of the VCF record, used as the reference uses them (0-based indices) */
    int32_t type;               /* IM_CLS_*                                            */
    int32_t alt_off, alt_len;   /* the ALT string in alts[]                            */
} im_known_variant;
typedef struct {
    int32_t variant;            /* index into variants[]                               */
    int32_t rstart, rstop;      /* 0 <= rstart <= rstop <= contig length               */
    int32_t q_off, q_len;       /* the aligned part of the read in queries[]           */
    int32_t own_subs, own_indels, own_aligned;      /* of the read's own alignment     */
    int32_t flags;              /* IM_SC_*                                             */
} im_count_task;
int im_support_count(im_ctx* ctx, int32_t n_variants, const im_known_variant* variants, const uint8_t* alts, int64_t alt_bytes,
                     int32_t n_tasks, const im_count_task* tasks, const uint8_t* queries, int64_t query_bytes,
                     int32_t* counts /* n_variants x 3 */);

/* ---- device-resident level --------------------------------------------- */

/* Device buffers of one realign batch.  All pointers are device pointers owned
 * by the caller (hipMalloc or a torch tensor's data_ptr).  bases must hold
 * each read at a 4-byte aligned offset (base_off[i] % 4 == 0) and 8 spare
 * bytes after the last read. */
typedef struct im_dev_batch {
    int32_t        n;
    const uint8_t* bases;
    const int64_t* base_off;    /* n   start of read i in bases, multiple of 4 */
    const int32_t* read_len;    /* n   */
    const int32_t* tid;
    const int32_t* anchor;
    const int32_t* range_max;
    im_read_result* out;        /* n   */
    /* optional evidence SLOT arrays, n * IM_MAX_EV entries each (NULL = not wanted):
     * slot i*IM_MAX_EV+k carries evidence k of read i, cls = -1 marks an empty slot.
     * Slot order is arrival order, so the arrays feed im_dev_cluster_groupby directly. */
    int32_t* ev_cls;
    int32_t* ev_b1;
    int32_t* ev_b2;
} im_dev_batch;

/* Launch the realign kernel on `stream` (a hipStream_t, NULL = default stream).
 * Asynchronous: returns after the launch. */
int im_dev_realign(im_ctx* ctx, const im_params* params,
                   const im_dev_batch* batch, void* stream);

/* The reference realigns reads of any length with a band of any width (src/readaln.c:242-267, src/indelminer.c:934,948).
 * Here reads of up to 255 bases run in the kernels laid out for them (four read positions per lane; numgaps <= 60: a lane
 * per band diagonal); reads of 256 .. IM_MAX_READ bases at numgaps == 0 (2 x 300 chemistry) take a second launch with
 * sixteen positions per lane; reads beyond IM_MAX_READ, reads beyond 255 bases with numgaps > 0, and every read when
 * numgaps > 60 take a general pass (one lane per read, its state in device memory; it synchronises the stream once and
 * cannot be captured into a launch graph).  Every im_dev_realign* call issues the later launches behind the first once the
 * context has been told that such reads occur: max_len = the longest read seen so far (the value only ever grows; callable
 * from any thread).  im_realign_batch (host buffers) calls it by itself.  Without the call a read beyond 255 bases comes
 * back IM_ST_UNSUPPORTED. */
int im_expect_read_length(im_ctx* ctx, int32_t max_len);

/* The results' trip to the host.  attempt_pe_alignment returns NULL for most candidates (src/alignment.c:764-799), and the
 * caller reads a candidate's 512-byte record only when it holds realigned evidence (src/indelminer.c:494-502): this packs the
 * records with status == IM_ST_EVIDENCE and n_ev > 0 into compact[] (capacity n records, order unspecified) and leaves per
 * read its status in status[i] and its place in compact[] -- or -1 -- in slot[i]; *count (a device int32, set by the call)
 * receives the number of packed records.  n_dev: device-resident batch size (NULL: n).  Asynchronous. */
int im_dev_compact_results(im_ctx* ctx, const im_read_result* res, int32_t n, const int32_t* n_dev,
                           int32_t* status, int32_t* slot, im_read_result* compact, int32_t* count, void* stream);

/* ---- seam 0: record triage -- fetch_func's candidate rules on the device ------- */

/* What fetch_func (src/indelminer.c:339-515) decides per delivered BAM record, done for a whole
 * chunk of records at once: the flag / pairing filters (348-366), the read-group lookup (369-376),
 * the three candidate cases with their mapping-quality gates (384-515), new_unaligned_readaln's
 * 4-bit -> ASCII decode and the reverse complement (src/readaln.c:242-267, src/indelminer.c:404-409,
 * 479-484), check_variants' CIGAR-derived evidence (285-337), and the read filter + match segments
 * of the DP= pileup (src/shared.c:160-176, bam_pileup.c:171-172).  Discordant pairs (516-615) stay
 * with the host's pair table; the kernel only labels them.
 *
 * Record classes (rec_class[], one byte per record): */
#define IM_REC_SKIP          0  /* returned before the read was counted (348-366)                */
#define IM_REC_COUNTED       1  /* counted (reaches 617), nothing to do                          */
#define IM_REC_CAND_UNMAPPED 2  /* unmapped read, mapped mate: realign (384-424)                 */
#define IM_REC_CAND_PROPER   3  /* proper pair with S/I/D: realign (425-515)                     */
#define IM_REC_PE            4  /* not a proper pair, passes 519-521: the host's readpairs path  */
#define IM_REC_ERR_RG       16  /* read group not in the insert-length table (must_find_hashtable exits) */
#define IM_REC_ERR_MQ       17  /* MQ tag of an unmapped read is not an integer (forceassert 395-397) */
#define IM_REC_ERR_CIGAR    18  /* N/H/P or unknown CIGAR op in a proper pair (new_readseg_bam exits) */
#define IM_REC_ERR_CLIP     19  /* soft clip inside the CIGAR (forceassert in check_variants, 325) */
#define IM_REC_ERR_BASE     20  /* base code outside A,C,G,T,N in a candidate (bit2char exits)   */
#define IM_REC_ERR_LIMIT    21  /* more than IM_MAX_EV CIGAR-derived evidence, or a malformed record */

/* the read-group -> range[1] table with the reference's hashtable semantics (16 bins, chains in
 * prepend order, prefix match, last hit wins: src/hashtable.c:62-81, src/hashfunc.c:23-30).
 * names[] in the ORDER THEY WERE ADDED to the table (config file order / first-seen order). */
int im_set_insert_ranges(im_ctx* ctx, int32_t n, const char* const* names, const int32_t* range_max);

/* A chunk of delivered records on the device: each record is the 32-byte BAM core followed by its
 * variable part (qname, cigar, seq, qual, aux) exactly as in the file, WITHOUT the block_size word,
 * starting at a 4-byte aligned offset.  A record whose core carries bin = 0xFFFF (no bin of any record: bins end at 37449)
 * comes WITHOUT its l_seq quality bytes -- (qname, cigar, seq, aux): nothing on the path reads qualities, and they are half
 * of every record's bytes over PCIe and out of HBM.  The deliverer may only leave them out when the CIGAR's read bases do not
 * exceed l_seq (the reference reads on behind the packed bases otherwise, src/readaln.c:186-240).  rec_off has n + 1 entries; record i spans rec_off[i]..rec_off[i+1], which may
 * include up to three bytes of alignment padding behind the aux area: the tag walk treats a tail shorter than the
 * smallest possible field (tag, type, one value byte = 4 bytes) as the end of the record.  The buffer behind `raw` must stay
 * readable for 64 bytes past the last record (the kernels read whole 16-byte pieces and a short look-ahead). */
typedef struct im_dev_records {
    int32_t         n;
    const uint8_t*  raw;
    const uint32_t* rec_off;
    int32_t         rec_base;   /* index of record 0 in the caller's numbering (goes into cand_rec) */
} im_dev_records;

typedef struct im_triage_params {
    int32_t  qthreshold;            /* -q */
    uint32_t ethreshold_vcfcheck;   /* -n (0 in annotate mode, src/indelminer.c:1074) */
    uint32_t maxpedelsize;          /* -p */
    int32_t  want_depth;            /* scatter the pileup match segments into the genome-wide difference array */
    int32_t  defer_ranges;          /* 1: the insert-length table is not known yet (it is being estimated in the same pass over the BAM):
                                     * no read-group look-up, range_max[] is left 0 for the caller to fill in, and EVERY pair that passes the
                                     * other tests of the discordant rule is labelled IM_REC_PE (the caller applies |isize| > range[1]) */
    int32_t  restart;               /* 1: this call opens a new batch -- counters[0..4] count as zero whatever they hold (saves the
                                     * caller a memset launch per batch); 0: the call appends to the running counters */
} im_triage_params;

/* Candidate batch under construction.  Candidates are APPENDED in record order: counters[0] = candidates
 * so far, counters[1] = read bytes so far (both updated by every call), counters[2] = records counted,
 * counters[3] = records with an IM_REC_ERR_* class.  batch holds the device arrays (capacity cap_cand
 * reads / cap_bases bytes); batch.n is ignored.  The evidence slots of a candidate receive its
 * CIGAR-derived evidence (check_variants); im_dev_realign later REPLACES them when the realignment
 * finds evidence (src/indelminer.c:494-512) -- launch it with keep_slots = 1 (im_dev_realign_keep).
 *
 * Overflow.  A candidate with index ci and base offset bo (the padded lengths of the candidates in front of it) is
 * ACCEPTED iff  ci < cap_cand  and  bo + padded4(l_seq) + 16 <= cap_bases  (16 bytes of slack behind the last read for the
 * realign kernels' whole-piece loads).  bo only grows, so the accepted candidates are a prefix of the batch.  Every candidate
 * that is refused adds 1 to counters[4] (zero after a call with restart = 1; else zero it with the other counters); nothing
 * of it is written: no bases, no scalars, no slots, no cand_rec -- except that one refused for its bytes below cap_cand gets
 * read_len 0 and base_off 0.  counters[0] and counters[1] still count the refused candidates, so min(counters[0], cap_cand)
 * bounds the entries that hold anything.  A caller that sees counters[4] != 0 must drop the batch (or repeat it with larger
 * buffers): the accepted prefix is right, the rest is missing. */
typedef struct im_dev_cands {
    im_dev_batch batch;
    int32_t*     cand_rec;      /* cap_cand: record index (rec_base + i) of every candidate      */
    int32_t*     counters;      /* device int32[8]; zero it before the first call (im_dev_alloc does not) */
    uint8_t*     rec_class;     /* n records of the chunk (may be NULL)                          */
    int32_t      cap_cand;
    int64_t      cap_bases;
    int32_t*     consumed;      /* optional: the flush marks of the evidence slots (im_dev_flush_*); a new candidate's
                                   IM_MAX_EV marks are cleared here, so that no separate fill is needed per batch    */
} im_dev_cands;

size_t im_dev_triage_scratch_bytes(int32_t n_records);
/* once per scratch buffer, before its first use (asynchronous; the launches leave it ready for the next one) */
int im_dev_triage_scratch_init(im_ctx* ctx, int32_t n_records, void* scratch, size_t scratch_bytes, void* stream);
int im_dev_triage(im_ctx* ctx, const im_triage_params* tp, const im_dev_records* recs,
                  const im_dev_cands* out, void* scratch, size_t scratch_bytes, void* stream);

/* im_dev_realign that leaves the evidence slots of reads WITHOUT realigned evidence untouched (the
 * CIGAR-derived evidence im_dev_triage put there survives, as at src/indelminer.c:504-510). */
int im_dev_realign_keep(im_ctx* ctx, const im_params* params, const im_dev_batch* batch, void* stream);
/* the same with the batch size read from DEVICE memory (*n_dev, e.g. counters[0] of im_dev_cands), so that no host
 * round trip sits between triage and realignment; batch->n is the upper bound the launch is sized for. */
int im_dev_realign_n(im_ctx* ctx, const im_params* params, const im_dev_batch* batch, const int32_t* n_dev, int32_t keep_slots, void* stream);

/* ---- seam 2, streaming form: the READCHUNK flushes on the device ---------------- */

/* process_evidence's node selection (src/indelminer.c:123-146) for one flush: among the PENDING
 * entries (cls >= 0, consumed[] == 0) of up to two slot ranges, the entries that sort before the
 * first (b1,b2)-sorted entry with b2 >= marker become graph nodes: consumed[slot] = flush_id (> 0).
 * Range A = split-read evidence slots, range B = the host's paired-read evidence (cls = 2), which
 * takes part in the cut but is clustered on the host.  cut_word: one device uint64 PER FLUSH, set to
 * all ones beforehand (it receives the (b1,b2) of the cutting entry).  Asynchronous. */
int im_dev_flush_cut(im_ctx* ctx, const int32_t* cls, const int32_t* b1, const int32_t* b2, int32_t* consumed,
                     int32_t a0, int32_t a1, int32_t b0, int32_t b1_end,
                     int32_t marker, int32_t flush_id, uint64_t* cut_word, void* stream);
/* the same with range A given as RECORD bounds [rec0, rec1): the slots of the candidates whose record index
 * (cand_rec[], ascending, *n_cand_dev of them, both on the device as im_dev_triage left them) lies inside --
 * the flush points are known to the host as record counts, the candidate list only to the device. */
int im_dev_flush_cut_rec(im_ctx* ctx, const int32_t* cls, const int32_t* b1, const int32_t* b2, int32_t* consumed,
                         int32_t rec0, int32_t rec1, const int32_t* cand_rec, const int32_t* n_cand_dev, int32_t cand_cap,
                         int32_t b0, int32_t b1_end, int32_t marker, int32_t flush_id, uint64_t* cut_word, void* stream);

/* Every flush of a batch of contigs in ONE launch, in list order (the order of the file): desc[f] gives flush f's
 * record bounds [rec0, rec1) (records of its contig up to the flush point), its paired-read entries [pe0, pe1)
 * relative to slot pe_base, its marker and its id (> 0).  desc lives on the device.  A flush sees a few thousand
 * pending slots at the reference's READCHUNK, so one workgroup walks the list; callers with very long pending
 * ranges (no mid-contig flush ever consumes anything) use im_dev_flush_cut_rec per flush instead.
 * cls, b1, b2 and consumed are read a candidate (IM_MAX_EV slots = 16 bytes) at a time: their bases must be 16-byte aligned
 * (any im_dev_alloc / hipMalloc pointer is). */
typedef struct im_flush_desc {
    int32_t rec0, rec1, pe0, pe1, marker, id;
    int32_t last;               /* index (in the list) of the LAST flush of the same contig; read by im_dev_flush_groupby only */
    int32_t reserved;
} im_flush_desc;
int im_dev_flush_cuts(im_ctx* ctx, const im_flush_desc* desc_dev, int32_t n_flushes,
                      const int32_t* cls, const int32_t* b1, const int32_t* b2, int32_t* consumed,
                      const int32_t* cand_rec, const int32_t* n_cand_dev, int32_t cand_cap,
                      int32_t pe_base, int32_t pe_count /* their marks are cleared first */, void* stream);

/* The flush list AND the split-read group-by of a group of contigs in three chip-wide launches (the product's device
 * stage; im_dev_flush_cuts + im_dev_cluster_groupby are the sequential form of the same thing).
 *
 * Why no history is needed: find_marker (src/indelminer.c:211-233) is a minimum over the pair table, whose entries only
 * leave it or enter it at the current read position of a coordinate-sorted walk, and the marker of a flush is
 * min(that, current position) (622-623) -- so WITHIN A CONTIG THE MARKERS NEVER DECREASE (the end-of-contig flush has
 * INT_MAX, 806).  An entry a flush f' consumed sorted in front of f' s cutting entry, hence had b2 < marker(f') <=
 * marker(f) for every later flush f of the contig: it could not be f's cutting entry even if it were still pending.
 * So the cut of flush f is simply  cut(f) = min{ (b1,b2) of e : e arrived before f's bounds, b2(e) >= marker(f) }  over
 * ALL entries of the contig, and  consumed(e) = the first flush f at or after e's arrival with (b1,b2)(e) < cut(f).
 * Launch 1 gives every entry's key to the cuts of the (contiguous, usually empty) run of flushes it is a candidate
 * for; launch 2 marks every entry and enters the consumed split-read slots into the cluster table; launch 3 writes
 * each cluster's record and its members in arrival order.
 *
 * THE CALLER GUARANTEES: desc[] lists the flushes in file order, rec1 and pe1 never decrease along the list, the flushes
 * of one contig are consecutive, carry the index of the contig's last flush in `last`, and their markers never
 * decrease (true for every coordinate-sorted BAM; a caller that finds otherwise uses im_dev_flush_cuts).  Entries
 * that no flush of their contig consumes keep consumed = 0.  Outputs as im_dev_cluster_groupby; counts must be 8-byte
 * aligned; the slot arrays 16-byte aligned.  The scratch is prepared once (im_dev_flushgroup_scratch_init) for a slot
 * and a flush capacity and every call leaves it ready for the next one. */
size_t im_dev_flushgroup_scratch_bytes(int32_t n_slots_cap, int32_t n_flushes_cap);
int im_dev_flushgroup_scratch_init(im_ctx* ctx, int32_t n_slots_cap, int32_t n_flushes_cap, void* scratch, size_t scratch_bytes, void* stream);
int im_dev_flush_groupby(im_ctx* ctx, const im_flush_desc* desc_dev, int32_t n_flushes,
                         const int32_t* cls, const int32_t* b1, const int32_t* b2, int32_t* consumed,
                         const int32_t* cand_rec, const int32_t* n_cand_dev,
                         int32_t cand_cap /* also the launch bound.  cand_rec, cls, b1 and b2 must be READABLE up to cand_cap candidates
                                             (IM_MAX_EV slots each), whatever *n_cand_dev says: the kernels load a candidate beside the
                                             count and drop it when it lies behind it.  What stands there does not matter. */,
                         int32_t pe_base, int32_t pe_count, int32_t tie_desc,
                         int32_t* order, int32_t* cl_key, int32_t* cl_first, int32_t* cl_count, int32_t* counts,
                         void* scratch, size_t scratch_bytes, void* stream);

/* The split-read rule of add_node (src/graph.c:122-127) over every consumed slot of [0, n_slots):
 * one cluster per distinct (consumed flush, class, b1, b2).  Output: cl_key[4 * c] = {flush_id, cls, b1,
 * b2}, cl_first[c], cl_count[c] in no particular cluster order (the host orders the few clusters; the
 * per-evidence work is done here); order[] = slot indices, cluster after cluster, members ascending in
 * slot index (= arrival) or descending with tie_desc.  counts (device int32[2]) = {clusters, nodes}.
 * Entries with cls >= 2 are ignored. */
size_t im_dev_groupby_scratch_bytes(int32_t n_slots);
/* once per scratch buffer (asynchronous); every group-by call leaves the scratch ready for the next one.  The scratch is
 * laid out for THIS n_slots for its whole life: later calls may pass any n_slots up to it (the context remembers the
 * layout per scratch pointer; a scratch that was never initialised is refused) */
int im_dev_groupby_scratch_init(im_ctx* ctx, int32_t n_slots, void* scratch, size_t scratch_bytes, void* stream);
int im_dev_cluster_groupby(im_ctx* ctx, int32_t n_slots, const int32_t* cls, const int32_t* b1, const int32_t* b2,
                           const int32_t* consumed, int32_t tie_desc,
                           int32_t* order, int32_t* cl_key, int32_t* cl_first, int32_t* cl_count, int32_t* counts,
                           void* scratch, size_t scratch_bytes, void* stream);
/* n_slots = IM_MAX_EV * *n_cand_dev (device), at most n_slots_cap */
int im_dev_cluster_groupby_n(im_ctx* ctx, int32_t n_slots_cap, const int32_t* n_cand_dev,
                             const int32_t* cls, const int32_t* b1, const int32_t* b2,
                             const int32_t* consumed, int32_t tie_desc,
                             int32_t* order, int32_t* cl_key, int32_t* cl_first, int32_t* cl_count, int32_t* counts,
                             void* scratch, size_t scratch_bytes, void* stream);

/* ---- seam 3, genome-wide form ----------------------------------------------------- */

/* One int32 per reference position for ALL contigs (4 bytes per base of HBM), filled by im_dev_triage
 * (want_depth) as a difference array; im_depth_scan turns contig tid into depths once all its records
 * have been through triage (one launch: depths local to 8192-position tiles plus a tile offset each, which
 * only im_depth_query_tid knows how to read); im_depth_query_tid sums [beg,end) like im_depth_query. */
int im_depth_enable(im_ctx* ctx);
int im_depth_scan(im_ctx* ctx, int32_t tid, void* stream);
/* contig tid's run back to zeros (asynchronous): a contig that is to go through triage + im_depth_scan AGAIN */
int im_depth_reset(im_ctx* ctx, int32_t tid, void* stream);
int im_depth_query_tid(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* sum_out);
/* the same, and per query the DEEPEST position of [beg - 1, end] (max_out, may be NULL).  The depth array counts every record; samtools'
 * pileup, which the reference's DP= comes from (src/shared.c:178-212), stops buffering records that start at the position it stands on
 * once 8000 are buffered (src/samtools-0.1.19/bam_pileup.c:172,244): the host driver asks the file, with that rule, about the queries
 * whose maximum says the rule may have applied.
 * With a = max(beg, 0) and b = min(end, contig length): sum_out = the sum of depth[a .. b - 1]; max_out = the largest depth[p] over
 * p = (a > 0 ? a - 1 : a) .. (b < contig length ? b : b - 1).  A query with beg >= end, or one that does not meet the contig
 * (a >= b), answers sum 0 and an UNSPECIFIED maximum. */
int im_depth_query_max_tid(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* sum_out, uint32_t* max_out);
/* im_depth_median over contig tid's run of the genome-wide array, behind im_depth_scan: the lower median of min(depth, 4095)
 * over [beg, end) clipped to the contig, 0xFFFFFFFF for a query that is empty after the clip (the same definition, the same
 * saturation).  Like the sum, it counts every record -- samtools' 8000-record pileup cap does not apply to it. */
int im_depth_median_tid(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* med_out);
/* Multi-GPU, pieces of one contig walked by several ranks: every rank's difference array holds the +-1 of the records IT
 * delivered; their sum (one RCCL all-reduce over the whole array, before any im_depth_scan) is the single run's array.  The
 * reference has no counterpart (calculate_cov_params re-reads the file per variant, src/shared.c:178-212).  Synchronous. */
int im_depth_allreduce(im_ctx* ctx, im_comm* comm);

/* ---- seam 5: reference-spanning read counts, for genotype calls (-G) --------------- */

/* Replaces nothing in the reference: it prints NS= (reads that support the indel) and has no count of the reads that support the
 * REFERENCE allele at the same breakpoint (DP= is a mean pileup depth over a window and holds the NS= reads too).  The statistic:
 * a record is eligible iff its flag has none of 0x4 / 0x100 / 0x200 / 0x400 (the pileup's mask), its tid names a contig and its
 * mapping quality is >= min_mapq.  A RUN is a maximal sequence of consecutive M / = / X operations of its CIGAR, covering contig
 * positions [s, e) clipped to [0, length); D and N advance the position and end a run, every other operation ends a run without
 * advancing.  span[p], 0 <= p <= length, is the number of runs of eligible records with s <= p - flank and p + flank <= e: the
 * run holds `flank` matched bases on each side of the boundary in front of base p.
 *
 * Genome-wide form, beside seam 3's: im_span_enable allocates one int32 per reference position for all contigs (4 bytes per base
 * of HBM, on this call only; flank >= 1) and fixes flank and min_mapq; im_dev_span_scatter adds a chunk of delivered records (the
 * chunk im_dev_triage takes; a launch of its own, asynchronous) to the difference array; im_span_scan turns contig tid into
 * counts once all its records have been through the scatter (the depth array's tiled scan); im_span_reset puts contig tid's run
 * back to zeros; im_span_query_tid returns per query the MINIMUM of span[p] over [beg, end] INCLUSIVE, clipped to
 * [0, length] (0 for an interval that is empty after the clip). */
int im_span_enable(im_ctx* ctx, int32_t flank, int32_t min_mapq);
int im_dev_span_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream);
int im_span_scan(im_ctx* ctx, int32_t tid, void* stream);
int im_span_reset(im_ctx* ctx, int32_t tid, void* stream);
int im_span_query_tid(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* min_out);
/* Host-buffer form, beside im_depth_build / im_depth_query: once per contig the runs (contig start, length) of its eligible
 * records -- the caller applies the record rule and forms the runs -- leave span[] of that contig resident on the device;
 * im_span_query answers like im_span_query_tid.  Synchronous. */
int im_span_build(im_ctx* ctx, int64_t contig_len, int32_t n_run, const int32_t* run_start, const int32_t* run_len, int32_t flank);
int im_span_query(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* min_out);

/* Concordant pairs, for the records without a precise breakpoint (PAIRED_READ; -P).  Replaces nothing in the reference either.
 * With m = flank >= 1, q = min_mapq and range_max = range[1] of the record's read group (its RG:Z tag, "generic" without one:
 * the look-up of fetch_func, through the table of im_set_insert_ranges), a record is a CONCORDANT LEFT MATE iff
 *   flag & 0x1 is set and none of 0x4 | 0x8 | 0x100 | 0x200 | 0x400 | 0x800;
 *   0 <= tid < n_contigs and mtid == tid;
 *   ((flag >> 4) & 1) != ((flag >> 5) & 1), the orientation test of the discordant rule;
 *   isize > 0;  pos < mpos, or pos == mpos and flag & 0x40 (each pair once);  mapq >= q (the record's own);
 *   its read group is in the table and isize <= range_max, the complement of the evidence rule abs(isize) > range[1] (a record
 *   whose group is not in the table is skipped here: the triage of the same chunk ends the run on it).
 * Its FRAGMENT is [a, b) = [pos, pos + isize) clipped to [0, length).  pspan[p], 0 <= p <= length, counts the fragments with
 * a + m <= p and p + m <= b; as a difference array a fragment with b - a >= 2 m adds +1 at a + m and -1 at b - m + 1 -- the
 * shape of span[], scanned and queried by the same kernels.  The minimum of pspan[] over [POS, max(END, BP_END)] is the thinnest
 * concordant-fragment depth between the two breakpoints of a deletion: a lower bound of the pairs of the reference allele.
 *
 * The entries mirror seam 5's, with the same contracts: im_pairspan_enable allocates a SECOND array of one int32 per reference
 * position (4 more bytes per base of HBM, on this call only); im_dev_pairspan_scatter (a launch of its own, asynchronous) needs
 * im_set_insert_ranges and answers IM_E_ARG without it; scan, reset and query_tid as for span[].  im_pairspan_build takes the
 * fragments (start, length) of one contig's concordant left mates -- the caller applies the record rule -- and leaves pspan[] of
 * that contig resident beside, and independent of, what im_span_build made; im_pairspan_query answers like im_span_query. */
int im_pairspan_enable(im_ctx* ctx, int32_t flank, int32_t min_mapq);
int im_dev_pairspan_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream);
int im_pairspan_scan(im_ctx* ctx, int32_t tid, void* stream);
int im_pairspan_reset(im_ctx* ctx, int32_t tid, void* stream);
int im_pairspan_query_tid(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* min_out);
int im_pairspan_build(im_ctx* ctx, int64_t contig_len, int32_t n_frag, const int32_t* frag_start, const int32_t* frag_len, int32_t flank);
int im_pairspan_query(im_ctx* ctx, int32_t n, const int32_t* beg, const int32_t* end, uint32_t* min_out);

/* Clipped reads, the breakpoint evidence of large deletions (-C).  Replaces nothing in the reference either: it realigns a clipped
 * read only when the deletion is shorter than -s and looks at no clip beyond that.  Two POINT-COUNT arrays of the family's layout
 * (per contig length + 1 entries), never scanned.  With c = min_clip >= 1 and q = min_mapq, a record is ELIGIBLE iff
 *   its flag has none of 0x4 | 0x100 | 0x200 | 0x400 (the span scatter's mask);  0 <= tid < n_contigs;  mapq >= q;
 *   its CIGAR has at least one reference-consuming operation (M, =, X, D, N).
 * Let `first` be its first operation that is not H and `last` its last that is not H, and refend = pos + the lengths of its
 * M / = / X / D / N operations.  Then
 *   RIGHT CLIP: last is S with length >= c and 0 <= refend <= length:  clipR[refend] += 1  (the read stops aligning in front of refend);
 *   LEFT CLIP:  first is S with length >= c and 0 <= pos <= length:    clipL[pos] += 1     (the read starts aligning at pos).
 * A record can add to both arrays.  A record whose only operation that is not H is an S adds nothing (it consumes no reference).
 * An S anywhere else in the CIGAR is ignored here: the triage of the same chunk ends the run on it.  For a deletion of the
 * 0-based bases [a, b) the reads from the left pile up on clipR[a] and the reads from the right on clipL[b].
 *
 * QUERY: a side (0: clipR, 1: clipL) and an interval [beg, end] INCLUSIVE, clipped to [0, length].  The answer is the LARGEST
 * count in the interval and the SMALLEST position that holds it (an interval of zeros answers count 0 at its first position); an
 * interval that is empty after the clip answers count 0 and position -1.  side is given per query, so one call serves both sides
 * of every record of a flush.  A null pointer with n >= 1, or a side other than 0 and 1, is IM_E_ARG.
 *
 * im_clip_enable allocates both arrays for all contigs (8 bytes per reference base of HBM, on this call only; min_clip >= 1) and
 * fixes min_clip and min_mapq: a second call with other values is refused.  im_dev_clip_scatter adds a chunk of delivered records
 * (the chunk im_dev_triage takes, with or without base qualities; one launch of its own, asynchronous); there is no scan, the
 * arrays are counts as they stand once the scatters have completed.  im_clip_reset puts contig tid's run of both arrays back to
 * zeros.  Host-buffer form: im_clip_build takes one contig's events (position, side) -- the caller applies the record rule;
 * positions outside [0, contig_len] are dropped -- and leaves both arrays of that contig resident beside what the other builds
 * made; im_clip_query answers like im_clip_query_tid.  Synchronous. */
int im_clip_enable(im_ctx* ctx, int32_t min_clip, int32_t min_mapq);
int im_dev_clip_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream);
int im_clip_reset(im_ctx* ctx, int32_t tid, void* stream);
int im_clip_query_tid(im_ctx* ctx, int32_t tid, int32_t n, const uint8_t* side, const int32_t* beg, const int32_t* end, uint32_t* count_out, int32_t* pos_out);
int im_clip_build(im_ctx* ctx, int64_t contig_len, int32_t n, const int32_t* pos, const uint8_t* side);
int im_clip_query(im_ctx* ctx, int32_t n, const uint8_t* side, const int32_t* beg, const int32_t* end, uint32_t* count_out, int32_t* pos_out);

/* Facing piles, the breakpoints of large insertions (-I).  An insertion too long for a read to span leaves what a deletion leaves,
 * the other way round: the reads from the left align through pr - 1 and clip there (clipR[pr]), the reads from the right align from
 * pl and clip in front of it (clipL[pl]), and pl <= pr -- the stretch [pl, pr) is the target-site duplication, or the micro-homology
 * an aligner extended into.  A deletion has pl > pr and is never a facing pile.  Unlike every query above this one names no interval:
 * it SEARCHES a whole contig.  With m = min_reads >= 1 and T = max_overlap, 0 <= T <= 64, on a contig with R = clipR and L = clipL
 * (length + 1 entries each), position p in [0, length] is a FACING PILE iff
 *   R[p] >= m;
 *   p is a peak of R: R[p] > R[x] for every x in [p - T, p) and R[p] >= R[x] for every x in (p, p + T], both clipped to [0, length]
 *   (of equal peaks within reach of each other the leftmost is the pile: the family's "smallest position" rule);
 *   the largest L[x] over x in [p - T, p], clipped to [0, length], the largest x among equals (the smallest overlap), is >= m.
 * The answer per pile is pr = p, pl = that x, cr = R[p], cl = L[x].  The windows stop at the contig's own entries: the run of the next
 * contig in the genome-wide arrays never enters.  Piles come back sorted by pr ascending.  *n_found is ALWAYS the number of piles;
 * when it exceeds cap the call still returns IM_OK, the four arrays are unspecified and the caller asks again with a larger cap.
 * im_clip_facing_tid searches contig tid of the genome-wide arrays (im_clip_enable; the scatters must have completed),
 * im_clip_facing the arrays of the last im_clip_build.  A min_reads below 1, a max_overlap outside 0 .. 64, a negative cap, a null
 * n_found, or a null array with cap >= 1 is IM_E_ARG; the rest as for im_clip_query_tid.  Synchronous, on the context's stream. */
int im_clip_facing_tid(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t max_overlap, int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr,
                       uint32_t* cl, int32_t* n_found);
int im_clip_facing(im_ctx* ctx, int32_t min_reads, int32_t max_overlap, int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr, uint32_t* cl,
                   int32_t* n_found);

/* Clip tails, what the clipped reads were clipped OF (-V).  The counts above say where reads stop; an adapter, a chimera, an insertion
 * or an inversion leaves the same pile.  At a deletion of the 0-based bases [a, b) the clipped tail of a read from the left is the
 * reference from b on, and the clipped head of a read from the right is the reference in front of a.  A keyed table keeps the
 * clipped bases nearest the junction; a query compares them with the resident reference behind the partner breakpoint.
 *
 * WHICH RECORDS STORE AN ENTRY.  The record rule is the one above, unchanged: the same eligibility, the same first / last operation
 * apart from H, c = min_clip, q = min_mapq, refend and pos inside [0, length].  Read bases are counted from 0 in the record's packed
 * bases, codes as BAM packs them (A C G T = 1 2 4 8).
 *   RIGHT ENTRY at (tid, refend): a right clip of L >= c bases; n = min(L, 32); base i, i = 0 .. n - 1, is read base l_seq - L + i
 *                                 (base 0 is the first clipped base, the one nearest the junction);
 *   LEFT ENTRY at (tid, pos):     a left clip of L >= c bases;  n = min(L, 32); base i is read base L - 1 - i (the head, reversed:
 *                                 base 0 is again the one nearest the junction).
 * An entry is stored only if all its n codes are A, C, G or T and the bases lie inside the record's packed-base bytes: l_seq > 0,
 * L <= l_seq, and the (l_seq + 1) / 2 bytes behind the CIGAR end inside the record.  Otherwise nothing is stored for that side; an N
 * beyond the first n clipped bases does not matter.  The counts of clipR / clipL are not touched by any of this.  Both delivered
 * record forms are taken (im_dev_records): the packed bases sit behind the CIGAR with base qualities behind them or without.
 *
 * A QUERY is (tid, pr, pl), a right-clip position and a left-clip position in array coordinates (for the deletion [a, b): pr = a,
 * pl = b), with max_shift S, 0 <= S <= 32.  For a shift s = 0 .. S
 *   a right entry at (tid, pr) MATCHES iff at most n >> 4 of its n bases differ from what is expected: base i is ref[pl + s + i];
 *   a left entry at (tid, pl) MATCHES iff at most n >> 4 of its n bases differ from what is expected: base i is ref[pr - 1 - s - i].
 * A reference position outside [0, length) and a reference byte other than A, C, G, T (the resident reference is upper-cased ASCII)
 * are mismatches.  The shift is the micro-homology an aligner extends into before it clips: with deleted bases [a, b) and a homology
 * of h bases the piles stand at a + h and b, or at a and b - h, and both sides match at s = h.  vR(s) and vL(s) are the matching
 * entries of either side; the chosen s has the largest vR(s) + vL(s), the smallest shift among equals.  The answer is vR, vL and s of
 * that shift, and the numbers of entries stored at (tid, pr, right) and (tid, pl, left), whatever their bases.  A query with pl <= pr
 * answers 0, 0, -1; a best sum of 0 answers 0, 0, -1 as well.
 *
 * THE TABLE has 2^log2_slots slots of 16 bytes (6 <= log2_slots <= 30): a multimap with open addressing; the home slot of an entry
 * is ((key >> 6) * 0x9E3779B97F4A7C15) >> (64 - log2_slots) with key = 1 << 63 | tid << 39 | position << 7 | side << 6 | n, probing is
 * linear and wraps past the last slot.  Only half of the slots are ever taken: the number of entries stored is exactly
 * min(entries asked for, 2^log2_slots / 2) and the rest are counted as dropped.  Once dropped > 0 an answer could miss entries, so
 * im_cliptail_verify then returns IM_OK and fills EVERY output of the call with 0xFFFFFFFF (shift: -1): no answer, not a wrong one.
 *
 * im_cliptail_enable allocates the table (16 << log2_slots bytes of HBM, on this call only; the reference must be set, at most 2^24
 * contigs) and fixes min_clip >= 1 and min_mapq: a second call with other values is refused.  im_dev_cliptail_scatter adds the
 * entries of a chunk of delivered records (one launch of its own, asynchronous).  im_cliptail_add adds n entries of contig tid the
 * caller names -- it applies the record rule itself -- as position, side (0: right, 1: left), number of bases 1 .. 32 and
 * planes[2 i], planes[2 i + 1]: bit k of the first word is the low bit and of the second the high bit of base k's code A C G T =
 * 0 1 2 3 (bits from n on are ignored); positions outside [0, length] are dropped without counting; synchronous.  im_cliptail_verify
 * answers nq queries of contig tid; synchronous, on the context's stream.  im_cliptail_reset puts all slots and both counters back to
 * zero.  im_cliptail_stats gives the entries stored and dropped since the last reset; synchronous. */
int im_cliptail_enable(im_ctx* ctx, int32_t min_clip, int32_t min_mapq, int32_t log2_slots);
int im_dev_cliptail_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream);
int im_cliptail_add(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* pos, const uint8_t* side, const uint8_t* nbases, const uint32_t* planes);
int im_cliptail_verify(im_ctx* ctx, int32_t tid, int32_t nq, const int32_t* pr, const int32_t* pl, int32_t max_shift, uint32_t* v_right,
                       uint32_t* v_left, int32_t* shift, uint32_t* stored_right, uint32_t* stored_left);
int im_cliptail_reset(im_ctx* ctx, void* stream);
int im_cliptail_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped);

/* The consensus of a pile (-I): what the entries at one key say when compared with EACH OTHER, not with the reference -- at a facing
 * pile the right entries at pr hold the first bases of the inserted sequence and the left entries at pl its last ones.  A query is
 * (tid, pos, side), with min_cover c >= 1.  E = the entries stored at the key; entry e has n_e bases b_e[i], i = 0 nearest the junction.
 *   cover(i) = #{e : n_e > i} (it does not increase with i);  len = #{i < 32 : cover(i) >= c};
 *   for i < len, cons[i] = the base most entries hold at i, the smallest code (A < C < G < T) among equals;
 *   entry e AGREES iff it differs from cons in at most min(n_e, len) >> 4 of its first min(n_e, len) bases (the tolerance of verify).
 * The answer per query is entries = |E|, len, the consensus as the table's own two planes (planes[2 q]: low bits, planes[2 q + 1]: high
 * bits, codes A C G T = 0 1 2 3, bits from len on zero) and agree, which is 0 when len is 0.  Every output is independent of the order in
 * which the entries arrived.  A position outside [0, length] answers all zeros.  Once dropped > 0 every output of the call is
 * 0xFFFFFFFF, as for im_cliptail_verify.  A min_cover below 1 or a side other than 0 and 1 is IM_E_ARG.  The table is built for piles
 * of tens of reads: a pile of thousands of entries is one long probe run that every query of its neighbourhood walks twice here.
 * Synchronous, on the context's stream. */
int im_cliptail_consensus(im_ctx* ctx, int32_t tid, int32_t nq, const int32_t* pos, const uint8_t* side, int32_t min_cover, uint32_t* entries,
                          uint32_t* len, uint32_t* planes, uint32_t* agree);

/* Crossed piles, the breakpoints of tandem duplications (-U).  One arrangement of two piles is left that nothing above reads: a
 * right-clip pile at pr and a left-clip pile at pl with pl FAR IN FRONT of pr.  That is what a tandem duplication of the bases [pl, pr)
 * leaves: a read that runs off the end of the first copy continues at the start of the second, so its clipped tail is ref[pl ...], and a
 * read that enters the second copy from the first has a clipped head of ref[... pr - 1] -- the match rule of im_cliptail_verify to the
 * letter, which answers 0, 0, -1 for every pl <= pr, while the facing search looks no further than its max_overlap in front of a pile.
 * With m = min_reads >= 1, T = reach (0 .. 64), dmin = min_len >= 1, dmax = max_len >= dmin, S = max_shift (0 .. 32) and
 * mv = min_verified >= 1, on a contig of length clen:
 *   position p is a PEAK of an array A (clen + 1 entries) iff A[p] >= m, A[p] > A[x] for every x in [p - T, p) and A[p] >= A[x] for every
 *   x in (p, p + T], both windows clipped to [0, clen] -- the peak half of the facing rule, applied to clipR and to clipL alike; two
 *   peaks of one array are at least T + 1 apart;
 *   a CANDIDATE is a peak pr of clipR and a peak pl of clipL of the same contig with dmin <= pr - pl <= dmax;
 *   vR(s) = the right entries at (tid, pr) of which at most n >> 4 bases differ from ref[pl + s + i], vL(s) = the left entries at
 *   (tid, pl) of which at most n >> 4 differ from ref[pr - 1 - s - i]; positions outside [0, clen) and bytes other than A, C, G, T are
 *   mismatches (the rule of im_cliptail_verify, without its pl > pr condition);
 *   the chosen s has the largest vR(s) + vL(s) over 0 .. S, the smallest s among equals;
 *   a candidate QUALIFIES iff vR >= mv and vL >= mv at the chosen s.
 * The answer per qualifying pair is pr, pl, cr = clipR[pr], cl = clipL[pl], vR, vL, s and the entries stored at the two keys.  Pairs
 * come back sorted by (pr, pl); a peak may qualify with several partners (a repeat), and all of them are reported.  *n_found is
 * ALWAYS the number of qualifying pairs; when it exceeds cap the call still returns IM_OK, the arrays are unspecified and the caller
 * asks again with a larger cap.  Once the table has dropped entries *n_found = -1, nothing is written and the call returns IM_OK: no
 * answer, not a wrong one.
 * im_clip_peaks_tid / im_clip_peaks answer the peaks of ONE array, side 0 (clipR) or 1 (clipL), sorted by position, with the cap
 * contract above; apart from side their argument checks are those of im_clip_facing_tid / im_clip_facing.  im_clip_crossed_tid searches
 * contig tid of the genome-wide arrays, im_clip_crossed the arrays of the last im_clip_build, which must be contig tid's (the table is
 * keyed by contig and the reference is the contig's: the build form has to be told which).  Parameters outside the ranges above, a
 * negative cap, a null n_found or a null array with cap >= 1 are IM_E_ARG; so are clip arrays or a table that are not enabled and a
 * reference that is not set.  The candidates of a peak are walked one by one: max_len bounds them to max_len / (T + 1) + 1 per peak.
 * Synchronous, on the context's stream. */
int im_clip_peaks_tid(im_ctx* ctx, int32_t tid, int32_t side, int32_t min_reads, int32_t reach, int32_t cap, int32_t* pos, uint32_t* count,
                      int32_t* n_found);
int im_clip_peaks(im_ctx* ctx, int32_t side, int32_t min_reads, int32_t reach, int32_t cap, int32_t* pos, uint32_t* count, int32_t* n_found);
int im_clip_crossed_tid(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift,
                        int32_t min_verified, int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr, uint32_t* cl, uint32_t* v_right, uint32_t* v_left,
                        int32_t* shift, uint32_t* stored_right, uint32_t* stored_left, int32_t* n_found);
int im_clip_crossed(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift,
                    int32_t min_verified, int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr, uint32_t* cl, uint32_t* v_right, uint32_t* v_left,
                    int32_t* shift, uint32_t* stored_right, uint32_t* stored_left, int32_t* n_found);

/* Inverted piles, the breakpoints of inversions (-N).  Every rule above pairs a right-clip pile with a left-clip pile and compares the
 * clipped bases with the reference as it stands.  An inversion of the bases [a, b) -- the sample reads ref[0, a) + revcomp(ref[a, b)) +
 * ref[b, ...) -- leaves neither.  At its LEFT junction the reads that keep most of their bases in front of a stop aligning at a with a
 * right clip, and clipped base i is comp(ref[b - 1 - i]); the reads that keep most of their bases inside the inverted segment align on
 * the other strand, stop at b with a right clip, and clipped base i is comp(ref[a - 1 - i]): two RIGHT-clip piles, each holding the
 * complement of the reference running backwards from the other.  The RIGHT junction leaves two LEFT-clip piles at a and b that hold, in
 * junction order, comp(ref[b + i]) and comp(ref[a + i]).  Micro-homology the aligner extended into, h1 bases at one pile and h2 at the
 * other, moves the piles to a + h1 and b + h2 (right clips; a - h1 and b - h2 for left clips), and both piles then verify at the ONE
 * shift s = h1 + h2.  In the table's 2-bit planes (A 0, C 1, G 2, T 3) the complement is both planes inverted.
 * With m = min_reads >= 1, T = reach (0 .. 64), dmin = min_len >= 1, dmax = max_len >= dmin, S = max_shift (0 .. 32) and
 * mv = min_verified >= 1, on a contig of length clen:
 *   PEAK is the definition of "Crossed piles", unchanged;
 *   a CANDIDATE of side sigma (0 = clipR, 1 = clipL) is two peaks x < y of the SAME array with dmin <= y - x <= dmax;
 *   an entry of n bases matches iff at most n >> 4 of its bases differ from what is expected; a position outside [0, clen) is a
 *   mismatch, and so is a reference byte other than A, C, G, T.  Base i at shift s is expected to be
 *     sigma = 0, the entry at x:  comp(ref[y - 1 - s - i])        sigma = 0, the entry at y:  comp(ref[x - 1 - s - i])
 *     sigma = 1, the entry at x:  comp(ref[y + s + i])            sigma = 1, the entry at y:  comp(ref[x + s + i])
 *   v1(s) = the matching entries at (tid, x, sigma), v2(s) = the matching entries at (tid, y, sigma);
 *   the chosen s has the largest v1(s) + v2(s) over 0 .. S, the smallest s among equals;
 *   a candidate QUALIFIES iff v1 >= mv and v2 >= mv at the chosen s.
 * The answer per qualifying pair is side, x, y, c1 = A[x], c2 = A[y], v1, v2, s and the entries stored at the two keys.  Pairs come
 * back sorted by (x, y, side); a pair x < y is reported once, a peak may be the y of one pair and the x of another, and a peak may
 * qualify with several partners.  *n_found is ALWAYS the number of qualifying pairs, under the cap contract of im_clip_crossed_tid:
 * when it exceeds cap the call still returns IM_OK, the arrays are unspecified and the caller asks again with a larger cap.  Once the
 * table has dropped entries *n_found = -1, nothing is written and the call returns IM_OK: no answer, not a wrong one.
 * im_clip_inverted_tid searches contig tid of the genome-wide arrays, im_clip_inverted the arrays of the last im_clip_build, which must
 * be contig tid's.  Argument errors are those of the crossed entries: parameters outside the ranges above, a negative cap, a null
 * n_found or a null array with cap >= 1 are IM_E_ARG; so are clip arrays or a table that are not enabled and a reference that is not
 * set.  The two junctions of one inversion are two pairs, one of either side; nothing joins them here.  Synchronous, on the
 * context's stream. */
int im_clip_inverted_tid(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift,
                         int32_t min_verified, int32_t cap, uint8_t* side, int32_t* p1, int32_t* p2, uint32_t* c1, uint32_t* c2, uint32_t* v1,
                         uint32_t* v2, int32_t* shift, uint32_t* stored1, uint32_t* stored2, int32_t* n_found);
int im_clip_inverted(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift,
                     int32_t min_verified, int32_t cap, uint8_t* side, int32_t* p1, int32_t* p2, uint32_t* c1, uint32_t* c2, uint32_t* v1,
                     uint32_t* v2, int32_t* shift, uint32_t* stored1, uint32_t* stored2, int32_t* n_found);

/* Pair links, the read pairs that span a junction (-M).  The piles above are one kind of evidence, the clipped reads AT the two
 * breakpoints.  A second, independent one is the orientation of the pairs whose reads lie on either side of a junction: a tandem
 * duplication of [pl, pr) leaves EVERTED pairs (the leftmost read on the reverse strand near pl, its mate on the forward strand just in
 * front of pr), the left junction of an inversion leaves pairs with BOTH READS FORWARD, its right junction pairs with BOTH READS REVERSE.
 * A keyed table of its own, beside the clip-tail table, keeps one link per such pair; a query counts the links between two windows.
 *
 * WHICH RECORDS STORE A LINK.  With q = min_mapq a delivered record is a LINK iff all of
 *   flag & 0x1 is set and none of 0x4 | 0x8 | 0x100 | 0x200 | 0x400 | 0x800 is;
 *   0 <= tid < n_contigs and mtid == tid;
 *   pos < mpos, or pos == mpos and flag & 0x40 (each pair once, at its leftmost record: the rule of the pair-span scatter);
 *   mapq >= q (the record's own mapping quality; its mate's is not known);
 *   0 <= pos <= length and 0 <= mpos <= length of the contig;
 *   with r = (flag >> 4) & 1 and m = (flag >> 5) & 1 the pair (r, m) gives the KIND:
 *     (1, 0)  kind 0, EVERTED   the duplication signature
 *     (0, 0)  kind 1, FORWARD   the inversion's left junction
 *     (1, 1)  kind 2, REVERSE   the inversion's right junction
 *     (0, 1)  none              the normal orientation is NOT a link, whatever its insert size
 * hold.  Only the 32-byte core of the record is read, so both delivered record forms are taken (im_dev_records); no read group is
 * looked up.  A link stores (tid, kind, pos, mpos).
 *
 * A QUERY is (kind, a0, a1, b0, b1) on contig tid; the call also takes one min_sep >= 0.  Both intervals are inclusive and are clipped
 * to [0, length].  The answer is the number of stored links of that kind with a0 <= pos <= a1, b0 <= mpos <= b1 and
 * mpos - pos >= min_sep; an interval that is empty after the clip answers 0.  a1 - a0 above 65 535 before the clip is IM_E_ARG, and so
 * are a kind outside 0 .. 2 and a negative min_sep.  The answer does not depend on the order in which the links arrived.
 *
 * THE TABLE has 2^log2_slots slots of 16 bytes (6 <= log2_slots <= 30), the design of the clip-tail table: a multimap with open
 * addressing; the home slot of a link is (key * 0x9E3779B97F4A7C15) >> (64 - log2_slots) with
 * key = 1 << 63 | tid << 26 | (pos >> 8) << 2 | kind, so all links of one (tid, 256-base bucket, kind) lie on one probe run; the payload
 * is pos | mpos << 32; probing is linear and wraps past the last slot.  Only half of the slots are ever taken: the number of links
 * stored is exactly min(links asked for, 2^log2_slots / 2) and the rest are counted as dropped.  Once dropped > 0 an answer could miss
 * links, so im_pairlink_count then returns IM_OK and fills every count of the call with 0xFFFFFFFF: no answer, not a wrong one.  A
 * query walks one probe run per bucket of [a0, a1], at most 257; a bucket with thousands of links is one long probe run.
 *
 * im_pairlink_enable allocates the table (16 << log2_slots bytes of HBM, on this call only; the reference must be set, at most 2^24
 * contigs) and fixes min_mapq: a second call with other values is refused.  im_dev_pairlink_scatter adds the links of a chunk of
 * delivered records (one launch of its own, asynchronous).  im_pairlink_add adds n links of contig tid the caller names -- it applies
 * the record rule itself -- as pos, mpos and kind 0 .. 2; a link with a position outside [0, length] is dropped without counting;
 * synchronous.  im_pairlink_count answers nq queries of contig tid; synchronous, on the context's stream.  im_pairlink_reset puts all
 * slots and both counters back to zero.  im_pairlink_stats gives the links stored and dropped since the last reset; synchronous. */
int im_pairlink_enable(im_ctx* ctx, int32_t min_mapq, int32_t log2_slots);
int im_dev_pairlink_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream);
int im_pairlink_add(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* pos, const int32_t* mpos, const uint8_t* kind);
int im_pairlink_count(im_ctx* ctx, int32_t tid, int32_t nq, const uint8_t* kind, const int32_t* a0, const int32_t* a1, const int32_t* b0,
                      const int32_t* b1, int32_t min_sep, uint32_t* count_out);
int im_pairlink_reset(im_ctx* ctx, void* stream);
int im_pairlink_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped);

/* Mate links, the read pairs whose reads lie on TWO contigs (-T).  Everything above stops at the contig's edge: the pile pairs are of
 * one contig and a pair link needs mtid == tid.  A junction between two contigs -- a translocation -- leaves a clip pile on either
 * contig and a bundle of pairs with one read near each.  A third keyed table, beside the clip-tail and the pair-link table, keeps one
 * link per READ of such a pair, and a query asks where the mates of the reads around a position lie: without it every pile would have
 * to be tried against every pile of every other contig.
 *
 * WHICH RECORDS STORE A LINK.  With q = min_mapq a delivered record is a MATE LINK iff all of
 *   flag & 0x1 is set and none of 0x4 | 0x8 | 0x100 | 0x200 | 0x400 | 0x800 is;
 *   0 <= tid < n_contigs, 0 <= mtid < n_contigs and mtid != tid;
 *   mapq >= q (the record's own mapping quality; its mate's is not known);
 *   0 <= pos <= length[tid] and 0 <= mpos <= length[mtid]
 * hold.  EVERY such record stores one link at its own contig: there is no leftmost-read rule, the two reads of a pair store one link
 * each, and a query from either contig finds the pair.  kind = r | m << 1 with r = (flag >> 4) & 1 (this read reverse) and
 * m = (flag >> 5) & 1 (its mate reverse): four kinds, 0 .. 3.  A link is (tid, kind, pos, mtid, mpos).  Only the 32-byte core of the
 * record is read, so both delivered record forms are taken (im_dev_records); no read group is looked up.
 *
 * A PARTNER QUERY is (kind, a0, a1) on contig tid.  The interval is inclusive and is clipped to [0, length]; a1 - a0 above 65 535 before
 * the clip is IM_E_ARG, and so is a kind outside 0 .. 3.
 *   L = the stored links of contig tid and that kind with a0 <= pos <= a1;
 *   the CELL of a link is (mtid, mpos >> 10);
 *   score(mtid, c) = the number of links of L in the cells (mtid, c) and (mtid, c + 1);
 *   the WINNER is the (mtid, c) of the largest score; among equals the smallest mtid wins, then the smallest c.
 * Two neighbouring cells span 2 048 bases, so a bundle of mates within some 1 000 bases of each other is always inside one pair of
 * cells, wherever the cell borders fall.  The answer per query is n_links = |L|, mtid, n_partner = the winner's score, and lo, hi = the
 * smallest and the largest mpos among the winner's links (those of L in its two cells).  |L| = 0 answers mtid = -1 and zeros.  A query
 * keeps at most IM_MATELINK_CELLS = 256 distinct cells: one whose links lie in more answers mtid = -2, n_partner = lo = hi = 0, with
 * n_links still exact -- no answer, not a wrong one (a pile in a repeat, whose mates scatter over the genome).  Whether that happens
 * depends on the set of links alone; no output depends on the order in which the links arrived.
 *
 * THE TABLE has 2^log2_slots slots of 16 bytes (6 <= log2_slots <= 30), the design of the other two: a multimap with open addressing;
 * the home slot of a link is (key * 0x9E3779B97F4A7C15) >> (64 - log2_slots) with key = 1 << 63 | tid << 26 | (pos >> 8) << 2 | kind, so
 * all links of one (tid, 256-base bucket, kind) lie on one probe run; the payload is (pos & 255) | mtid << 8 | mpos << 32; probing is
 * linear and wraps past the last slot.  Only half of the slots are ever taken: the number of links stored is exactly
 * min(links asked for, 2^log2_slots / 2) and the rest are counted as dropped.  Once dropped > 0 an answer could miss links, so
 * im_matelink_partner then returns IM_OK and fills EVERY output of the call with 0xFFFFFFFF (mtid, lo, hi: -1): no answer, not a wrong
 * one.  A query walks one probe run per bucket of [a0, a1], at most 257.
 *
 * im_matelink_enable allocates the table (16 << log2_slots bytes of HBM, on this call only; the reference must be set, at most 2^24
 * contigs) and fixes min_mapq: a second call with other values is refused.  A new reference frees it with the other keyed tables.
 * im_dev_matelink_scatter adds the links of a chunk of delivered records (one launch of its own, asynchronous); without
 * im_matelink_enable it is IM_E_ARG with a message.  im_matelink_add adds n links of contig tid the caller names as pos, mtid, mpos and
 * kind 0 .. 3; it applies the rule's range checks itself: a link with mtid outside [0, n_contigs), mtid == tid or a position outside
 * [0, length] of its contig is dropped without counting; synchronous.  im_matelink_partner answers nq queries of contig tid;
 * synchronous, on the context's stream.  im_matelink_reset puts all slots and both counters back to zero.  im_matelink_stats gives the
 * links stored and dropped since the last reset; synchronous. */
#define IM_MATELINK_CELLS 256
int im_matelink_enable(im_ctx* ctx, int32_t min_mapq, int32_t log2_slots);
int im_dev_matelink_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream);
int im_matelink_add(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* pos, const int32_t* mtid, const int32_t* mpos, const uint8_t* kind);
int im_matelink_partner(im_ctx* ctx, int32_t tid, int32_t nq, const uint8_t* kind, const int32_t* a0, const int32_t* a1, uint32_t* n_links,
                        int32_t* mtid_out, uint32_t* n_partner, int32_t* lo, int32_t* hi);
int im_matelink_reset(im_ctx* ctx, void* stream);
int im_matelink_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped);

/* Junctions, the clip tails of one pile against ANOTHER CONTIG (-T), and the one statement of the four verify rules above.  A query is
 * two ends (tid1, p1, side1) and (tid2, p2, side2) with max_shift S, 0 <= S <= 32; a side is 0 = the right clips piled up at the
 * position, 1 = the left clips.  The two contigs may be the same, and there is NO condition on the order of the positions.
 * An entry at end A, of n bases, base 0 nearest the junction, is compared with the reference at the OTHER end (tidB, pB, sideB): for a
 * shift s = 0 .. S its base i is expected to be
 *   sideB = 1:  refB[pB + s + i]          (the other end's reads were clipped on their left: its contig goes on forwards from pB)
 *   sideB = 0:  refB[pB - 1 - s - i]      (clipped on their right: its contig runs backwards from the base in front of pB)
 * and, iff sideA == sideB, the COMPLEMENT of that reference byte (two piles of one side join the two strands).  The entry MATCHES iff
 * at most n >> 4 of its n bases differ from what is expected; a position outside [0, length[tidB]) and a reference byte other than
 * A, C, G, T (the resident reference is upper-cased ASCII) are mismatches.  v1(s), v2(s) are the matching entries at end 1 and end 2;
 * the chosen s has the largest v1(s) + v2(s) over 0 .. S, the smallest s among equals.  The answer is v1, v2 and s of that shift and
 * stored1, stored2, the numbers of entries stored at the two keys, whatever their bases; a best sum of 0 answers 0, 0, -1; an end whose
 * position lies outside [0, length] has no entry.  Once the clip-tail table has dropped entries every output of the call is
 * 0xFFFFFFFF (shift: -1).
 * With tid1 == tid2 this is, to the letter: im_cliptail_verify for (pr, 0) and (pl, 1) with pl > pr; the crossed rule for (pr, 0) and
 * (pl, 1) with pl < pr; the inverted rules for (x, sigma) and (y, sigma).  A contig outside 0 .. n_contigs - 1, a side other than 0 and
 * 1, S outside 0 .. 32, a negative nq or a null array with nq >= 1 is IM_E_ARG; so are a table that is not enabled and a reference that
 * is not set.  Synchronous, on the context's stream. */
int im_cliptail_junction(im_ctx* ctx, int32_t nq, const int32_t* tid1, const int32_t* p1, const uint8_t* side1, const int32_t* tid2, const int32_t* p2,
                         const uint8_t* side2, int32_t max_shift, uint32_t* v1, uint32_t* v2, int32_t* shift, uint32_t* stored1, uint32_t* stored2);

/* Split links, the reads an aligner has split at a junction (-S).  The piles and the pairs above are indirect: 32 clipped bases compared
 * with the reference, and the orientation of pairs whose mate's mapping quality is not known.  A read that CROSSES a junction is written
 * by a split aligner as a primary record with a soft clip, and its SA:Z tag says where the clipped part was placed: contig, position,
 * strand, CIGAR and that placement's own mapping quality.  A fourth keyed table keeps one link per such record, from the junction end
 * its clip marks to the junction end the tag names -- the ends (tid, position, side) of im_cliptail_junction -- and a query counts the
 * links between two ends.
 *
 * WHICH RECORDS STORE A LINK.  With c = min_clip >= 1 and q = min_mapq a delivered record stores AT MOST ONE split link, iff all of
 *   THE FRONT  the core is whole (32 bytes, l_seq >= 0, and the CIGAR and the start of the aux area inside the record); the flag has
 *     none of 0x4 | 0x100 | 0x200 | 0x400 | 0x800 (each read once, at its primary record; paired or not does not matter);
 *     0 <= tid < n_contigs; mapq >= q;
 *   THE CIGAR  has at least one reference-consuming operation (-C's eligibility); first, last = its first and last operation that is
 *     not H; refend = pos + the lengths of its M = X D N; L1, T1 = the total lengths of its leading and its trailing run of H and S;
 *   THE TAG  the aux area holds an SA tag; the FIRST occurrence is taken, found by samtools' walk (bam_aux_get: fixed sizes for
 *     A c C s S i I f d, Z and H to their NUL, B by its header; an unknown type or a field that runs out of the record ends the walk;
 *     a tail of fewer than 4 bytes is padding); its type is Z; it is NUL-terminated inside the record; and its value is EXACTLY ONE
 *     entry  rname,pos,strand,cigar,mapQ,NM  followed by ';' NUL or by NUL alone, with
 *       rname   1 or more bytes, none of ',' ';' NUL
 *       pos     1 to 10 decimal digits, value 1 .. 2^31 - 1 (1-based)
 *       strand  '+' or '-'
 *       cigar   one or more of (1 to 9 digits, then one of MIDNSHP=X)
 *       mapQ    1 to 3 digits
 *       NM      1 or more digits (value unused)
 *     anything else -- a second entry, an empty field, a non-digit, a tag of another type -- stores nothing;
 *   THE SA ALIGNMENT  tid2 = the contig whose name equals rname byte for byte over its whole length (no prefix match; an unknown name
 *     stores nothing); p2 = pos - 1; span2 = the sum of its M = X D N lengths (64 bits), span2 >= 1; e2 = p2 + span2 <= length[tid2];
 *     its mapQ >= q; L2, T2 = the length of its first and of its last operation when that is S or H, else 0;
 *     same = ((strand == '-') == ((flag >> 4) & 1)); when !same, L2 and T2 are swapped (the entry's CIGAR is written for the other strand);
 *   WHICH SIDE  BEHIND iff L2 > L1 and T2 < T1 (the other part holds the read's bases behind the primary's); FRONT iff L2 < L1 and
 *     T2 > T1; neither (a tie in either) stores nothing;
 *   END A, the primary's   BEHIND: last is S of >= c bases and 0 <= refend <= length[tid]: A = (tid, refend, 0), -C's RIGHT CLIP;
 *                          FRONT:  first is S of >= c bases and 0 <= pos <= length[tid]:   A = (tid, pos, 1),    -C's LEFT CLIP;
 *     so a split link always sits on a position and side that clipR or clipL counted;
 *   END B, the other part's            same strand       other strand
 *                          BEHIND      (tid2, p2, 1)     (tid2, e2, 0)
 *                          FRONT       (tid2, e2, 0)     (tid2, p2, 1)
 * hold.  The link is (tidA, pA, sideA, tidB, pB, sideB), kind = sideA | sideB << 1; tidB == tidA is allowed.  Both delivered record
 * forms are taken (im_dev_records).
 *
 * WORKED EXAMPLES, a read of 100 bases whose primary record is forward on contig tid at x (0-based), the other part on ctgB:
 *   60M40S, SA:Z:ctgB,p,+,60S40M,60,0;   BEHIND, same strand:   A = (tid, x + 60, 0)  B = (ctgB, p - 1, 1)       kind 2  ("3to5": a deletion, a duplication)
 *   60M40S, SA:Z:ctgB,p,-,40M60S,60,0;   BEHIND, other strand:  A = (tid, x + 60, 0)  B = (ctgB, p - 1 + 40, 0)  kind 0  ("3to3": an inversion's left junction)
 *   40S60M, SA:Z:ctgB,p,+,40M60S,60,0;   FRONT, same strand:    A = (tid, x, 1)       B = (ctgB, p - 1 + 40, 0)  kind 1  ("5to3")
 *   40S60M, SA:Z:ctgB,p,-,60S40M,60,0;   FRONT, other strand:   A = (tid, x, 1)       B = (ctgB, p - 1, 1)       kind 3  ("5to5": an inversion's right junction)
 *
 * A QUERY is (tid1, side1, a0, a1, tid2, side2, b0, b1).  Both intervals are inclusive and are clipped to [0, length] of their contig.
 * The answer is the number of stored links with tidA == tid1, kind == side1 | side2 << 1, a0 <= pA <= a1, tidB == tid2 and
 * b0 <= pB <= b1; an interval that is empty after the clip answers 0.  a1 - a0 above 65 535 before the clip, a side other than 0 or 1,
 * a contig outside the reference, or a null array with nq >= 1 is IM_E_ARG.  No answer depends on the order in which the links arrived.
 *
 * THE TABLE has 2^log2_slots slots of 16 bytes (6 <= log2_slots <= 30), the design of the other three: a multimap with open addressing;
 * the home slot of a link is (key * 0x9E3779B97F4A7C15) >> (64 - log2_slots) with key = 1 << 63 | tidA << 26 | (pA >> 8) << 2 | kind, so
 * all links of one (tidA, 256-base bucket, kind) lie on one probe run; the payload is (pA & 255) | tidB << 8 | pB << 32; probing is
 * linear and wraps.  Only half of the slots are ever taken: the number stored is exactly min(links asked for, 2^log2_slots / 2) and the
 * rest are counted as dropped.  Once dropped > 0 im_splitlink_count returns IM_OK and fills every count of the call with 0xFFFFFFFF:
 * no answer, not a wrong one.  A query walks one probe run per bucket of [a0, a1], at most 257.
 *
 * im_splitlink_enable allocates the table (16 << log2_slots bytes of HBM, on this call only) and fixes min_clip, min_mapq and the contig
 * names: the reference must be set, n_names must equal its number of contigs, and names[i] is contig i's name as the BAM header spells
 * it.  A null or empty name, two equal names, min_clip < 1 and log2_slots outside 6 .. 30 are IM_E_ARG with a message; a second call
 * with other values is refused.  A new reference frees the table with the other three.  im_dev_splitlink_scatter adds the links of a
 * chunk of delivered records (one launch of its own, asynchronous); without im_splitlink_enable it is IM_E_ARG with a message.
 * im_splitlink_add adds n links the caller names as six columns; it applies the rule's range checks itself: a link with a contig
 * outside the reference or a position outside [0, length] of its contig is dropped without counting (a side other than 0 or 1 is
 * IM_E_ARG); synchronous.  im_splitlink_count answers nq queries; synchronous, on the context's stream.  im_splitlink_reset puts all
 * slots and both counters back to zero.  im_splitlink_stats gives the links stored and dropped since the last reset; synchronous. */
int im_splitlink_enable(im_ctx* ctx, int32_t min_clip, int32_t min_mapq, int32_t log2_slots, int32_t n_names, const char* const* names);
int im_dev_splitlink_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream);
int im_splitlink_add(im_ctx* ctx, int32_t n, const int32_t* tid, const int32_t* pos, const uint8_t* side, const int32_t* tid2, const int32_t* pos2,
                     const uint8_t* side2);
int im_splitlink_count(im_ctx* ctx, int32_t nq, const int32_t* tid1, const uint8_t* side1, const int32_t* a0, const int32_t* a1,
                       const int32_t* tid2, const uint8_t* side2, const int32_t* b0, const int32_t* b1, uint32_t* count_out);
int im_splitlink_reset(im_ctx* ctx, void* stream);
int im_splitlink_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped);

/* Split junctions, the junctions the split links name BY THEMSELVES (-J).  Every search above starts from two piles of clipped reads
 * on one position each and compares clipped bases with the reference; im_splitlink_count only counts links for a record found that
 * way.  A junction with inserted bases, with more micro-homology than 32 bases, or whose reads were clipped at scattered positions has
 * no such record, though every read across it stores a link that names both ends to the base.  This search reads the table alone.
 *
 * A stored link is L = (tA, pA, sA, tB, pB, sB).  rev(L) = (tB, pB, sB, tA, pA, sA).  can(L) = L when (tA, pA, sA) <= (tB, pB, sB)
 * in lexicographic order, rev(L) otherwise; a canonical tuple is written (t1, p1, s1, t2, p2, s2).  With W = window (0 .. 255),
 * min_span >= 0 and min_links >= 1:
 *   1. CANDIDATES  a stored link is a candidate iff tA != tB or |pA - pB| >= min_span (a smaller event is an indel: stdout's); a
 *      candidate junction is a distinct value c = can(L) of a candidate link;
 *   2. EXACT SUPPORT  E(c) = the number of stored links equal to c or to rev(c) (a link equal to both counts once);
 *   3. NEAR  two candidate junctions c, c' are near iff t1, s1, t2, s2 are equal and |p1 - p1'| <= W and |p2 - p2'| <= W;
 *   4. PEAK  c is a peak iff no near candidate junction c' BEATS it; c' beats c on the larger E, among equal E on the smaller p1, then
 *      on the smaller p2.  This is non-maximum suppression, the peak rule of "Crossed piles" in two dimensions, and like it NOT
 *      transitive: a candidate suppressed by a neighbour that is itself suppressed stays suppressed;
 *   5. COUNTS  n1 of a peak is, by definition, what im_splitlink_count answers for (t1, s1, p1 - W, p1 + W, t2, s2, p2 - W, p2 + W) and
 *      n2 what it answers with the two ends exchanged; EVERY stored link counts, candidate or not;
 *   6. THRESHOLD  a peak with n1 + n2 < min_links is dropped, after the suppression: it un-suppresses nothing;
 *   7. ORDER  the answer is the remaining peaks, each once, sorted by (t1, p1, t2, p2, s1, s2).
 * No answer depends on the order in which the links arrived or on the slots that hold them.
 *
 * WORKED EXAMPLE, W = 32, min_span = 50, min_links = 3, the links stored (contig 0 throughout):
 *   3 x (0, 1000, 0, 0, 5000, 1)   2 x (0, 5000, 1, 0, 1000, 0)   2 x (0, 1020, 0, 0, 5010, 1)   1 x (0, 1040, 0, 0, 5030, 1)
 *   1 x (0, 1010, 0, 0, 1030, 1)
 * The last link spans 20 bases: no candidate.  The second group is the reverse of the first: c1 = (0, 1000, 0, 0, 5000, 1) has
 * E = 5; c2 = (0, 1020, 0, 0, 5010, 1) has E = 2; c3 = (0, 1040, 0, 0, 5030, 1) has E = 1.  c1 and c2 are near (20, 10), c2 and c3 are
 * near (20, 20), c1 and c3 are not (40 > W).  c1 beats c2, c2 beats c3: c1 is the one peak, and c3 stays suppressed although the
 * junction that beats it is suppressed itself.  n1 of c1 counts the links from [968, 1032] side 0 to [4968, 5032] side 1: 3 + 2 = 5 (the
 * short link ends at 1030, outside); n2 counts those from [4968, 5032] side 1 to [968, 1032] side 0: 2.  The answer is the one row
 * (0, 1000, 0, 0, 5000, 1), E = 5, n1 = 5, n2 = 2.
 *
 * im_splitlink_junctions answers the whole table in one call: synchronous, on the context's stream, behind what is queued there.
 * *found is ALWAYS the number of junctions; when it exceeds cap nothing is written and the caller asks again with a larger cap (the
 * idiom of im_clip_peaks_tid).  Once the table has dropped links *found = -1, nothing is written and the call returns IM_OK: no
 * answer, not a wrong one.  window outside 0 .. 255, min_links < 1, min_span < 0, cap < 0, a null found, a null column with cap >= 1
 * and a table that im_splitlink_enable has not made are IM_E_ARG with a message.  The call allocates its workspace (12 bytes per
 * stored link, 4 per slot of the table, the columns) and frees it: it is meant to be made once per run.  A site with n links is n
 * walks of a probe run of n. */
int im_splitlink_junctions(im_ctx* ctx, int32_t window, int32_t min_links, int32_t min_span, int32_t cap, int32_t* tid1, int32_t* pos1, uint8_t* side1,
                           int32_t* tid2, int32_t* pos2, uint8_t* side2, uint32_t* exact, uint32_t* n1, uint32_t* n2, int32_t* found);

/* Junction genotypes (-K): a junction of im_splitlink_junctions against the reads that run through its two ends on the reference allele.
 * Both halves are on the device already.  For a junction (t1, p1, s1, t2, p2, s2, E, n1, n2), in array coordinates:
 *   ALT = n1 + n2.  A read stores ONE link, at its primary record's end, so the two window counts are disjoint sets of reads: their sum
 *     is the number of reads of the junction allele.
 *   RS1 = span[t1][p1] and RS2 = span[t2][p2], of the genome-wide array of this seam's first family (im_span_enable's flank and
 *     min_mapq).  The boundary in front of base p is where a right clip at refend = p and a left clip at pos = p both put the junction:
 *     span[p] counts the runs with `flank` matched bases on either side of exactly that boundary.  A split read's own run ends there,
 *     so it is in neither.
 *   RS = min(RS1, RS2), except for a tandem duplication (JT=DUP: one contig, s1 = 1, s2 = 0), where RS = max(0, min(RS1, RS2) - ALT).
 *     A tandem duplication leaves both outer boundaries of the duplicated segment intact ON THE DUPLICATED ALLELE: every copy of that
 *     allele adds reference-looking reads at p1 and at p2 at the rate at which it adds junction reads.  Uncorrected, a homozygous
 *     duplication shows RS ~ ALT and could never be called 1/1; the correction takes away as many reads as the junction has.
 *   (GT, GQ) are the genotype columns' own integers from (RS, ALT): in thousandths of a phred L(0/0) = ALT * 20000 + RS * 44,
 *     L(0/1) = (ALT + RS) * 3010, L(1/1) = ALT * 44 + RS * 20000; GT is the smallest (the lower index wins a tie), GQ the distance to
 *     the second smallest, rounded to whole phreds, at most 99.
 *
 * WORKED EXAMPLE, 10 reads per allele copy.  A heterozygous deletion junction (0, 1000, 0, 0, 1500, 1) with n1 = 5, n2 = 5 and
 * span[1000] = 10, span[1500] = 12: ALT = 10, RS = min(10, 12) = 10, L = (200440, 60200, 200440): GT 0/1, GQ 99.  A homozygous tandem
 * duplication (0, 3000, 1, 0, 3400, 0) with n1 = 10, n2 = 10 and span[3000] = span[3400] = 20 (both copies of the allele, reads through
 * either outer boundary): ALT = 20, RS = max(0, 20 - 20) = 0, L = (400000, 60200, 880): GT 1/1, GQ 59.  Without the correction RS would
 * be 20 and L = (400880, 120400, 400880): 0/1 at GQ 99, for a sample that has no reference allele at all.
 *
 * im_span_query_ends answers the reference side for a whole file of junctions in one launch: for every k, min_out[k] is the minimum of
 * span[p] of contig tid[k] over [pos[k] - slack, pos[k] + slack] clipped to [0, length] -- by definition what
 * im_span_query_tid(ctx, tid[k], 1, &beg, &end, ..) answers for that interval, which takes one contig per call.  Synchronous, on the
 * context's stream, behind what is queued there; every contig asked about must have been through im_span_scan (a contig that no record
 * was scattered to answers 0 scanned or not).  n == 0 is IM_OK without a launch.  n < 0, slack outside 0 .. 255, a null column with
 * n > 0, a tid outside the reference, a pos outside [0, length] and an array that im_span_enable has not made are IM_E_ARG with a
 * message that names the first offending end; the ranges are checked on the host before anything is copied.
 *
 * Limits of the genotype: a reference read must hold `flank` bases on either side while a split read needs a clip of min_clip bases and
 * a placed remainder, so the two alleles are not equally detectable and nothing corrects for it; RS is exact for one position while
 * micro-homology lets an aligner place the split anywhere inside it; span[] counts runs, so a read with an indel near the end may count
 * on neither side; the two junctions of an inversion or of a reciprocal translocation are genotyped independently. */
int im_span_query_ends(im_ctx* ctx, int32_t n, const int32_t* tid, const int32_t* pos, int32_t slack, uint32_t* min_out);

/* Junction overlap (-H): how many read bases the two parts of a split read share, or how many lie between them.  A junction of
 * im_splitlink_junctions says where its two ends are; what sets it apart from the junctions the pile searches report -- inserted or
 * non-templated bases, micro-homology beyond 32 bases -- is in no column of it.  Yet every read it counts carries that number exactly,
 * in the two CIGARs a split link is made from.  The table's 16-byte slot is full, so the number lives in an array of its own beside the
 * table: one uint16_t per slot, 0 = unknown, otherwise d + 32768.
 *
 * THE OVERLAP d OF A SPLIT LINK, in the names of "Split links" (L1, T1 the primary's clipped runs; L2, T2 the entry's, AFTER the swap
 * for the other strand):
 *   Q1 = L1 + T1 + the lengths of the primary CIGAR's M I = X operations   (the read's length as the primary record states it)
 *   Q2 = the lengths of the entry's M I S H = X operations                 (the same as the SA entry states it)
 *   Q1 != Q2:  d is unknown (the two do not describe one read)
 *   BEHIND:    d = (Q1 - T1) - L2   (the primary's part ends at read base Q1 - T1, the other part starts at L2)
 *   FRONT:     d = (Q1 - T2) - L1   (the other part ends at read base Q1 - T2, the primary's starts at L1)
 *   d outside -32767 .. 32767:  d is unknown
 * d > 0: the two parts share d read bases (micro-homology); d < 0: -d read bases belong to neither part (inserted bases); d = 0: a
 * clean junction.  I counts as read bases, D and N and P do not.  d is what the aligner says: nothing is compared with the reference.
 *
 * WORKED EXAMPLES, a read of 100 bases (primary CIGAR, SA entry, d):
 *   60M40S   ctgB,p,+,60S40M,60,0;   d = 0
 *   65M35S   ctgB,p,+,60S40M,60,0;   d = 5
 *   55M45S   ctgB,p,+,65S35M,60,0;   d = -10
 *   40S60M   ctgB,p,+,40M60S,60,0;   d = 0
 *   60M40S   ctgB,p,-,40M60S,60,0;   d = 0
 * (the last one on the other strand: L2, T2 = 60, 40 after the swap).
 *
 * im_splitlink_overlap_enable allocates the array (2 << log2_slots bytes of HBM) and clears it.  It comes behind im_splitlink_enable and
 * in front of the first link -- or behind im_splitlink_reset: while the table's counter of links asked for is not 0 it is IM_E_ARG with
 * a message.  A second call is IM_OK.  A new reference frees the array together with the table; im_splitlink_reset clears it.  From then
 * on im_dev_splitlink_scatter writes every link's d to the slot the link claimed.  WHICH links are stored and both
 * counters do not depend on the array: im_splitlink_stats, im_splitlink_count and im_splitlink_junctions answer what they answer without.
 * im_splitlink_add_overlap is im_splitlink_add with a seventh column: d[i] in -32767 .. 32767, or -32768 for unknown; IM_E_ARG with a
 * message when the array is not enabled.  A link added through im_splitlink_add has no d: it stays unknown.
 *
 * im_splitlink_overlap sums the array up for n junctions, the rows of im_splitlink_junctions.  For row k let D be the known d of every
 * stored link that the two count queries of rule 5 of "Split junctions" count: the links im_splitlink_count counts for
 * (tid1, side1, pos1 - window, pos1 + window, tid2, side2, pos2 - window, pos2 + window) and for the same with the two ends exchanged,
 * intervals clipped as it clips them; a link that both queries count (they can meet only where both ends share contig and side and the
 * windows overlap) is taken once.  Then
 *   known[k]  = |D|
 *   median[k] = the LOWER median: the element of index (|D| - 1) / 2 of D sorted in ascending order; 0 when D is empty
 *   agree[k]  = the number of elements of D equal to median[k] (0 when D is empty)
 * exactly, for any number of links.  Once the table has dropped links all three columns are filled with 0xFF bytes and the call returns
 * IM_OK: no answer, not a wrong one.  n == 0 is IM_OK without a launch.  n < 0, window outside 0 .. 255, a null column with n > 0, a side
 * other than 0 or 1, a contig outside the reference, a table that im_splitlink_enable has not made and an array that
 * im_splitlink_overlap_enable has not made are IM_E_ARG.  One launch, a wave per junction; synchronous, on the context's stream, behind
 * what is queued there.  No answer depends on the order in which the links arrived or on the slots that hold them.
 *
 * Limits: no inserted sequence (that needs read bases, which the table does not keep); no confidence interval; a read with an indel or
 * a mismatch inside the micro-homology is given whatever split its aligner chose. */
int im_splitlink_overlap_enable(im_ctx* ctx);
int im_splitlink_add_overlap(im_ctx* ctx, int32_t n, const int32_t* tid, const int32_t* pos, const uint8_t* side, const int32_t* tid2, const int32_t* pos2,
                             const uint8_t* side2, const int16_t* d);
int im_splitlink_overlap(im_ctx* ctx, int32_t n, const int32_t* tid1, const int32_t* pos1, const uint8_t* side1, const int32_t* tid2, const int32_t* pos2,
                         const uint8_t* side2, int32_t window, uint32_t* known, int32_t* median, uint32_t* agree);

/* Junction pairs (-E): the read pairs on either side of a junction of im_splitlink_junctions.  Its SE and SR are both counted from the
 * same split reads; a chimeric read or an aligner artefact gives the same picture.  The read pairs whose insert spans the junction
 * come from other molecules: an independent kind of evidence.  Both pair tables are on the device already ("Pair links", "Mate links");
 * two things were missing.  The commonest junction, a deletion's, leaves pairs in the NORMAL orientation that are too far apart, which
 * the pair links drop; and no query answers junctions with ends on arbitrary contigs in one call.
 *
 * THE STRETCHED PAIRS, kind 3 of the pair-link table.  The key's kind field has two bits and value 3 was free: the layout of the table
 * is what it was.  A delivered record is a link of kind 3, STRETCHED, iff it passes every line of WHICH RECORDS STORE A LINK of "Pair
 * links" down to the positions (paired, none of 0x4 0x8 0x100 0x200 0x400 0x800, mtid == tid, the leftmost-record rule, mapq >= q, both
 * starts in [0, length]), its orientation is (r, m) = (0, 1), and flag & 0x2 (proper pair) is CLEAR.  Only the 32-byte core is read;
 * no read group and no insert range is looked up: the aligner's own verdict stands in for the insert-size test.  A deletion shorter
 * than the spread of the library's insert size therefore leaves proper pairs and no link.
 *
 * im_pairlink_stretched_enable switches the rule on.  It comes behind im_pairlink_enable and in front of the first link -- or behind
 * im_pairlink_reset: while the table's links stored + dropped is not 0 it is IM_E_ARG with a message.  A second call is IM_OK.
 * im_pairlink_reset keeps the switch; a new reference drops it with the table.  From then on im_dev_pairlink_scatter stores the kind-3
 * links as well, and im_pairlink_add and im_pairlink_count take kind 3; without the switch kind 3 is the IM_E_ARG it was.  The links
 * of kinds 0 .. 2, the contents of their slots and both counters do not depend on the switch, but for the tickets the kind-3 links take.
 *
 * AN END is (t, p, s), s as everywhere: 0 = right clips (the reads lie in front of p, on the forward strand), 1 = left clips (the reads
 * lie behind p, on the reverse strand).  Its WINDOW is W(p, s) = s ? [p - back, p + reach] : [p - reach, p + back], inclusive, clipped
 * to [0, length[t]]: the windows of -M and -T.  A read that supports the end starts inside W and has strand s.
 *
 * im_junction_pairs answers n junctions (tid1, pos1, side1, tid2, pos2, side2), the rows of im_splitlink_junctions:
 *   tid1 == tid2   out of the pair-link table.  lo is the end with the smaller position (end 1 on a tie), hi the other;
 *                  kind = K(s_lo, s_hi) with K(1,0) = 0, K(0,0) = 1, K(1,1) = 2, K(0,1) = 3;
 *                  pe1 = the stored links of that kind with pos in W(lo), mpos in W(hi) and mpos - pos >= min_sep; pe2 = 0.
 *                  For kinds 0 .. 2 this is, to the letter, what im_pairlink_count answers for the same windows.
 *   tid1 != tid2   out of the mate-link table.  pe1 = the links stored at tid1 of kind s1 | s2 << 1 with pos in W(end 1), mtid == tid2
 *                  and mpos in W(end 2); pe2 = the same from end 2, kind s2 | s1 << 1.  min_sep does not apply.
 * An end whose window is empty after the clip answers 0.  Once the pair-link table has dropped links every answer of the call with
 * tid1 == tid2 is 0xFFFFFFFF in both columns, and once the mate-link table has, every answer with tid1 != tid2: per table, no answer,
 * not a wrong one; the other class still answers.
 *
 * WORKED EXAMPLES, reach 1000, back 32, min_sep 50, on contigs of 100 000 bases (junction; the pairs that count, as the leftmost
 * record's strand and start -> its mate's):
 *   DEL       (0, 5000, 0, 0, 5400, 1)   kind K(0,1) = 3: forward in [4000, 5032] -> reverse in [5368, 6400], flag 0x2 clear, >= 50 apart
 *   DUP       (0, 5000, 1, 0, 5400, 0)   kind K(1,0) = 0: reverse in [4968, 6000] -> forward in [4400, 5432], >= 50 apart
 *   INV 3to3  (0, 5000, 0, 0, 9000, 0)   kind K(0,0) = 1: forward in [4000, 5032] -> forward in [8000, 9032]
 *   INV 5to5  (0, 5000, 1, 0, 9000, 1)   kind K(1,1) = 2: reverse in [4968, 6000] -> reverse in [8968, 10000]
 *   TRA       (0, 5000, 0, 1, 7000, 1)   pe1: at contig 0, kind 0 | 1 << 1 = 2, forward in [4000, 5032], mate on contig 1 in [6968, 8000];
 *                                        pe2: at contig 1, kind 1 | 0 << 1 = 1, reverse in [6968, 8000], mate on contig 0 in [4000, 5032]
 * (one pair of the TRA junction stores a mate link at either contig, so it is counted in pe1 by one record and in pe2 by the other).
 *
 * IM_E_ARG with a message that names the junction's index: a contig outside the reference, a side other than 0 and 1; with a message:
 * reach < 0 or back < 0, reach + back > 65 535, min_sep < 0, n < 0, a null array with n >= 1, a pair-link table that is not enabled or
 * not in the stretched form, a mate-link table that is not enabled.  n == 0 is IM_OK without a launch.  One launch, a wave per
 * junction; synchronous, on the context's stream, behind what is queued there.  No answer depends on the order in which the links
 * arrived or on the slots that hold them.
 *
 * Limits: the proper-pair flag is the aligner's; the mate's mapping quality is not known; a duplication or an inversion shorter than a
 * read leaves no such pair; nothing is compared with an insert-size distribution. */
int im_pairlink_stretched_enable(im_ctx* ctx);
int im_junction_pairs(im_ctx* ctx, int32_t n, const int32_t* tid1, const int32_t* pos1, const uint8_t* side1, const int32_t* tid2, const int32_t* pos2,
                      const uint8_t* side2, int32_t reach, int32_t back, int32_t min_sep, uint32_t* pe1, uint32_t* pe2);

/* ---- multi-GPU: one collective ------------------------------------------------ */

/* Contigs are independent (the reference's own parallel mode is one process per -c
 * region, src/indelminer.c:536-542), so ranks own disjoint contigs and exchange
 * nothing until each holds its cluster list; then ONE all-gather (RCCL over xGMI).
 * Rendezvous: rank 0 calls im_comm_unique_id and ships the IM_COMM_ID_BYTES to the
 * other ranks by any side channel (bench.py: torch.distributed/gloo broadcast). */
#define IM_COMM_ID_BYTES 128
int  im_comm_unique_id(void* id_bytes);
int  im_comm_init(im_ctx* ctx, const void* id_bytes, int rank, int world, im_comm** out);
/* every rank contributes bytes_per_rank bytes; recv_dev holds world * bytes_per_rank.  Asynchronous. */
int  im_comm_allgather(im_comm* comm, const void* send_dev, void* recv_dev, size_t bytes_per_rank, void* stream);
/* in place: buf[i] = sum over ranks of buf[i].  Asynchronous. */
int  im_comm_allreduce_sum_i32(im_comm* comm, int32_t* buf_dev, size_t count, void* stream);
/* Point-to-point traffic of one exchange step, device memory to device memory over RCCL (xGMI): n operations issued as ONE group.
 * Operation k SENDS bytes[k] bytes at dev[k] to rank peer[k] (dir[k] = 0) or RECEIVES them from it (dir[k] = 1).  Every rank passes
 * the operations it takes part in, all ranks in the same global order (the host driver: walked groups in claim order, a group's host
 * part in front of its device arrays), so that sends and receives pair up whatever the ranks' timing.  Asynchronous.
 * Replaces nothing in the reference (it has no communication: src/indelminer.c:536-542); it is how a group walked by one rank
 * reaches the rank that owns its contig. */
int  im_comm_exchange(im_comm* comm, int32_t n, const int32_t* dir, const int32_t* peer, void* const* dev, const size_t* bytes, void* stream);
void im_comm_destroy(im_comm* comm);
const char* im_comm_last_error(void);

/* ---- device memory / timing plumbing for callers without a HIP binding --- */

/* hipMalloc / hipFree / hipMemcpy on the context's device.  im_dev_upload and
 * im_dev_download are synchronous. */
int  im_dev_alloc(im_ctx* ctx, size_t bytes, void** out);
int  im_dev_free(im_ctx* ctx, void* p);
int  im_dev_upload(im_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int  im_dev_download(im_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int  im_dev_memset(im_ctx* ctx, void* dst_dev, int byte, size_t bytes, void* stream);     /* asynchronous */
/* Pinned host memory and asynchronous copies on a stream ("reads are pre-staged into pinned buffers and
 * hipMemcpyAsync'd"): the host driver inflates BAM records straight into im_host_alloc'd chunks. */
int  im_host_alloc(im_ctx* ctx, size_t bytes, void** out);
int  im_host_free(im_ctx* ctx, void* p);
int  im_dev_upload_async(im_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes, void* stream);
int  im_dev_download_async(im_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes, void* stream);
int  im_dev_copy_async(im_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes, void* stream);
/* The context's own stream (a hipStream_t) and a wait for it. */
void* im_ctx_stream(im_ctx* ctx);
int   im_ctx_device(im_ctx* ctx);                               /* the HIP device index the context lives on */
int  im_stream_sync(im_ctx* ctx, void* stream);
/* HIP-event stopwatch on a stream: create, record start / stop on the stream the
 * kernels are launched on, read the elapsed milliseconds (synchronises on stop). */
typedef struct im_timer im_timer;
int  im_timer_create(im_ctx* ctx, im_timer** out);
void im_timer_destroy(im_timer* t);
int  im_timer_start(im_timer* t, void* stream);
int  im_timer_stop(im_timer* t, void* stream);
int  im_timer_elapsed_ms(im_timer* t, float* ms);

/* A second stream and stream-to-stream events, so that the cluster kernels of one flush can run while the
 * next flush's realign kernel does (two sets of realign output buffers; the reference has no counterpart,
 * its flushes are sequential host code, src/indelminer.c:617-640). */
typedef struct im_event im_event;
int  im_stream_create(im_ctx* ctx, void** out);
int  im_stream_destroy(im_ctx* ctx, void* stream);
int  im_event_create(im_ctx* ctx, im_event** out);
void im_event_destroy(im_event* ev);
int  im_event_record(im_event* ev, void* stream);
int  im_event_sync(im_event* ev);                               /* host waits */
int  im_stream_wait_event(im_ctx* ctx, void* stream, im_event* ev);
int  im_stream_follow(im_event* ev, void* from, void* to);      /* record on `from`, `to` waits */

/* Launch graphs.  One flush is a fixed sequence of dependent im_dev_* launches on one stream
 * (the reference has no counterpart: its flush, src/indelminer.c:617-640, is host code).  Between
 * im_capture_begin and im_capture_end the im_dev_* calls on `stream` are recorded instead of run;
 * im_graph_launch replays them with a single host call.  Device buffers and sizes are baked in:
 * capture again when they change. */
typedef struct im_graph im_graph;
int  im_capture_begin(im_ctx* ctx, void* stream);
int  im_capture_end(im_ctx* ctx, void* stream, im_graph** out);
int  im_graph_launch(im_graph* g, void* stream);
void im_graph_destroy(im_graph* g);

#ifdef __cplusplus
}
#endif
#endif
