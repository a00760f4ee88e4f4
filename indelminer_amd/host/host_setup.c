/* host_setup.c -- part of the indelminer host driver (one translation unit: imhost.c includes the parts in order, so that the
 * reference-shaped helpers can stay static).  Here: start-up: the GPU context thread, config file / insert-length estimation, the mean-coverage table, the VCF preamble, and
 * the record-at-a-time path (pass A / GPU / pass B per contig) that aborted runs are handed to. */

/* ------------------------------------------------------ GPU start-up ------- */

static void* gpu_open_thread(void* arg)
{
    driver* d = (driver*)arg;
    const char* dev_env = getenv("INDELMINER_DEVICE");
    d->gpu_rc = im_ctx_create(dev_env ? atoi(dev_env) : (g_mg_local >= 0 ? g_mg_local : 0), &d->gpu);
    if (d->gpu_rc != IM_OK) snprintf(d->gpu_err, sizeof d->gpu_err, "cannot open the GPU: %s", im_last_error(NULL));
    pthread_mutex_lock(&d->gpu_mu);
    d->ctx_rc = d->gpu_rc;
    d->ctx_ready = 1;                                   /* the walkers' buffers can be set up from here on */
    pthread_cond_broadcast(&d->gpu_cv);
    pthread_mutex_unlock(&d->gpu_mu);
    if (d->gpu_rc != IM_OK) return NULL;
    pthread_mutex_lock(&d->gpu_mu);
    while (!d->seq_ready) pthread_cond_wait(&d->gpu_cv, &d->gpu_mu);
    pthread_mutex_unlock(&d->gpu_mu);
    const char** seqs = xcalloc((size_t)d->hdr->n_targets, sizeof(char*));
    int64_t* lens = xcalloc((size_t)d->hdr->n_targets, sizeof(int64_t));
    for (int32_t i = 0; i < d->hdr->n_targets; i++) { seqs[i] = d->sequences[i] ? d->sequences[i] : ""; lens[i] = d->sequences[i] ? d->seqlen[i] : 0; }
    d->gpu_rc = im_set_reference(d->gpu, d->hdr->n_targets, seqs, lens);
    if (d->gpu_rc != IM_OK) snprintf(d->gpu_err, sizeof d->gpu_err, "im_set_reference: %s", im_last_error(d->gpu));
    free(seqs); free(lens);
    return NULL;
}

/* the output header (src/indelminer.c:745-754) */
static void print_output_header(void)
{
    if (strncmp(O.outputformat, "vcf", 3) == 0) print_vcf_preamble();
    if (g_vcfname != NULL)
        printf("##INFO=<ID=%s,Number=0,Type=Flag,Description=\"The variant is also present in this sample\">\n", g_sample_name);
    if (g_known_counts) {
        /* -A: no reference counterpart */
        printf("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype, the most likely of 0/0, 0/1, 1/1 given AD\">\n");
        printf("##FORMAT=<ID=AD,Number=2,Type=Integer,Description=\"Read support of the reference and the alternative allele in this sample: the smallest number, over the positions POS .. POS+(BP_END-END) the breakpoint can lie at, of alignments that match the reference for the -n distance on both sides of it, less those of them that support the indel; and the reads with mapping quality of at least -q that support the indel, by their CIGAR or by aligning at least as well against the reference with the indel applied\">\n");
        printf("##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: phred-scaled distance to the second most likely genotype, at most 99\">\n");
        if (g_pair_counts) printf("##pairedReadAD=\"PAIRED_READ records: AD = concordant pairs spanning the deletion with -n bases on each side (lower bound), pairs supporting it\"\n");
        printf("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n", g_sample_name);
    } else if (g_genotype) {
        /* -G: no reference counterpart */
        printf("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype, the most likely of 0/0, 0/1, 1/1 given AD\">\n");
        printf("##FORMAT=<ID=AD,Number=2,Type=Integer,Description=\"Read support of the reference and the alternative allele: the smallest number, over the positions POS .. POS+(BP_END-END) the breakpoint can lie at, of alignments that match the reference for the -n distance on both sides of it (an upper bound of the reads spanning the whole interval, exact when the interval is one position), and NS\">\n");
        printf("##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: phred-scaled distance to the second most likely genotype, at most 99\">\n");
        if (g_depth_evidence) {
            /* -D: no reference counterpart */
            printf("##FORMAT=<ID=DM,Number=3,Type=Integer,Description=\"Median depth over the deleted bases POS+1..END, over the %d bases in front of them and over the %d bases behind them\">\n", DEPTH_EV_FLANK, DEPTH_EV_FLANK);
            printf("##FORMAT=<ID=DFC,Number=1,Type=Integer,Description=\"Depth fold change in thousandths: the median inside the deletion over the mean of the flank medians\">\n");
        }
        if (g_clip_evidence) {
            /* -C: no reference counterpart */
            printf("##FORMAT=<ID=CB,Number=2,Type=Integer,Description=\"Breakpoints by clipped reads, in the coordinates of POS and END: where most soft-clipped reads stop aligning left of the deletion, and the base in front of where most start aligning right of it\">\n");
            printf("##FORMAT=<ID=CS,Number=2,Type=Integer,Description=\"Clipped reads at the two positions of CB\">\n");
            if (g_clip_verify) {
                /* -V: no reference counterpart */
                printf("##FORMAT=<ID=CV,Number=2,Type=Integer,Description=\"Of the clipped reads of CS, those whose clipped bases continue in the reference behind the other position of CB: left of the deletion, right of it\">\n");
                printf("##FORMAT=<ID=CH,Number=1,Type=Integer,Description=\"Bases of micro-homology (shift) at which the reads of CV continue\">\n");
            }
        }
        if (g_pair_counts) printf("##pairedReadAD=\"PAIRED_READ records: AD = concordant pairs spanning the deletion with -n bases on each side (lower bound), pairs supporting it\"\n");
        if (g_depth_evidence)
            printf("##depthEvidence=\"DELETION records with END-POS >= %d: DM = lower median (the smallest depth that at least half of the positions, rounded up, do not exceed) of the per-position depth over the deleted bases, the %d bases in front and the %d bases behind, each clipped to the contig, . for a flank without bases; DFC = 1000 * inside / mean of the flanks present, rounded, . without a flank or with flanks of depth 0. Depth = records samtools' pileup would count whose M/=/X covers the position, capped at 4095 per position; these are array counts without the pileup's limit of 8000 records, so DM can exceed what DP= implies at such loci\"\n",
                   DEPTH_EV_MIN_LEN, DEPTH_EV_FLANK, DEPTH_EV_FLANK);
        if (g_clip_evidence)
            printf("##clipEvidence=\"DELETION records with END-POS >= %d: a clipped read is an alignment samtools' pileup would count, with mapping quality of at least -q, whose first (last) CIGAR operation apart from hard clips is a soft clip of at least %d bases and whose CIGAR consumes reference; it counts at its first aligned base (left clip) or behind its last one (right clip). CS = the largest number of right clips on one position within %d positions of POS .. POS+(BP_END-END), and of left clips on one position within %d positions of END .. BP_END (PAIRED_READ records: both between POS-%d and max(END,BP_END)+%d); CB = the two positions, the smaller one among equal counts, printed so that a deletion whose clipped reads agree with the call shows its own POS,END; . and 0 for a side without clipped reads\"\n",
                   DEPTH_EV_MIN_LEN, CLIP_EV_MIN_CLIP, CLIP_EV_SLACK, CLIP_EV_SLACK, CLIP_EV_SLACK, CLIP_EV_SLACK);
        if (g_clip_verify)
            printf("##clipVerification=\"Records that carry CB:CS with both positions found and the second behind the first: of every clipped read counted there the %d clipped bases nearest the junction are kept (all of a shorter clip; a read with a base other than A, C, G, T among them is left out) and compared with the reference behind the other position, skipping s = 0 .. %d bases of micro-homology; a read is verified when at most n >> 4 of its n bases differ (1 of 16 .. 31, 2 of 32). CV = the verified reads left and right of the deletion at the s that verifies most, the smallest s among equals, CH = that s; 0,0 and . when none verifies; .,. and . for a record without both positions, and for every record once the table of clipped bases has overflowed (said on stderr at the end of the run)\"\n",
                   CLIPTAIL_BASES, CLIPTAIL_MAX_SHIFT);
        printf("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n", g_sample_name);
    } else if (strncmp(O.outputformat, "vcf", 3) == 0) printf("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n");
    fflush(OUT);
}
/* One pass without a config file: the reference prints its header after its estimation pass and the FASTA read -- a run it ends
 * inside that pass (an RG tag that is not a string) has printed nothing.  Here that pass IS the walk: the header waits until the
 * insert-length table has been made (run_pipeline). */
static int g_header_held;

/* the output header (src/indelminer.c:745-754); multi-GPU: rank 0 prints it, as the first part */
static void header_out(void)
{
    if (g_mg_rank > 0) return;
    if (g_mg_header_path[0] && !freopen(g_mg_header_path, "w", stdout)) fatalf("cannot write %s", g_mg_header_path);
    print_output_header();
    fflush(stdout);
    /* the header part is complete; whatever a library prints on stdout from here on (librccl's banner) is not VCF */
    if (g_mg_header_path[0] && !freopen("/dev/stderr", "w", stdout)) { }
}

/* every GPU call site passes through here first */
static void gpu_wait(driver* d)
{
    if (!d->gpu_pending) return;
    pthread_join(d->gpu_thread, NULL);
    d->gpu_pending = 0;
    if (d->gpu_rc != IM_OK) fatalf("%s", d->gpu_err);
    phase_time("GPU context + reference upload (helper thread, joined)");
    /* the output header (src/indelminer.c:745-754) goes out only once the GPU is known to be there:
     * nothing is printed by a run that cannot compute */
    if (g_header_held) return;
    header_out();
}

/* ------------------------------------------------------ config / estimates -- */

/* the insert-length table's entries in the order they were added: the device rebuilds the chains from it */
static const char** g_rg_name; static int32_t** g_rg_range; static int g_rg_n, g_rg_cap;
static void rg_order_push(const char* name, int32_t* range)
{
    if (g_rg_n == g_rg_cap) {
        g_rg_cap = g_rg_cap ? g_rg_cap * 2 : 16;
        g_rg_name = xrealloc(g_rg_name, sizeof(char*) * (size_t)g_rg_cap);
        g_rg_range = xrealloc(g_rg_range, sizeof(int32_t*) * (size_t)g_rg_cap);
    }
    g_rg_name[g_rg_n] = xstrdup(name); g_rg_range[g_rg_n] = range; g_rg_n++;
}

static uint32_t* g_meancov;         /* [n_targets] mean coverage: the RC lines of a config file, or observed (cov_means) */

static void read_configuration(const char* filename, qhash* insertlengths, const bam_header* hdr)
{
    /* src/shared.c:5-44.  An RC line's contig goes through must_find_hashtable_int on a 32-bin table of the BAM header's names
     * (src/indelminer.c:700-706) -- a name the header does not know ends the run there; the coverage itself is only ever
     * printed on stderr (src/indelminer.c:731). */
    qhash* id2chroms = qhash_new(5);
    for (int32_t i = 0; i < hdr->n_targets; i++) qhash_add(id2chroms, hdr->target_name[i], (int)strlen(hdr->target_name[i]), (void*)(intptr_t)(i + 1));
    if (!g_meancov) g_meancov = xcalloc((size_t)(hdr->n_targets > 0 ? hdr->n_targets : 1), sizeof(uint32_t));
    size_t cap = 2;
    char* line = xmalloc(cap);
    FILE* fp = fopen(filename, "r");
    if (!fp) fatalf("error in opening the file %s", filename);
    while (im_getline(&line, &cap, fp) != -1) {
        char name[128]; unsigned a, b;
        if (strncmp(line, "IL", 2) == 0) {
            if (sscanf(line, "IL %127s %u %u\n", name, &a, &b) != 3) fatalf("error in reading the insert length range: %s", line);
            int32_t* range = xmalloc(2 * sizeof(int32_t));
            range[0] = (int32_t)a; range[1] = (int32_t)b;
            qhash_add(insertlengths, name, (int)strlen(name), range);
            rg_order_push(name, range);
        } else if (strncmp(line, "RC", 2) == 0) {
            if (sscanf(line, "RC %127s %u\n", name, &a) != 2) fatalf("error in reading the mean coverage: %s", line);
            qbin* hit = qhash_lookup(id2chroms, name, (int)strlen(name));
            if (!hit) fatalf("did not find %s in the hash", name);
            g_meancov[(intptr_t)hit->val - 1] = a;
        } else fatalf("unknown tag in configuration: %s", line);
    }
    free(line);
    fclose(fp);
    qhash_free(id2chroms, NULL);
}

/* ---- observed coverage per contig (estimate_average_coverage, src/bamoperations.c:88-147) ---------------------------
 * The reference pileups every contig once more and prints floor(sum of the pileup's n / positions with n > 0) on stderr
 * (src/indelminer.c:728-733); nothing else reads the number.  The pileup's n at a position is the number of records -- not
 * unmapped, secondary, QC-fail or duplicate (BAM_DEF_MASK) -- whose reference span [pos, bam_calend) holds the position,
 * deletions and skips included: the sum is the sum of the spans, the covered positions are the union of the spans.  Both
 * come out of any walk of the records in file order: a running segment per walker, closed where the next record starts
 * behind its end; the few segments of all walkers are merged at the end.  (Not kept: the pileup buffer's cap of 8000
 * records starting at one position, bam_pileup.c.) */
typedef struct { int32_t tid, beg, end; } covseg;
typedef struct { int32_t nt; uint64_t* sum; covseg* seg; int64_t n, cap; int open; covseg cur; } covlist;
static uint32_t* g_meancov;         /* [n_targets]: from the RC lines of a config file, or observed */

static void cov_init(covlist* c, int32_t nt) { memset(c, 0, sizeof *c); c->nt = nt; c->sum = xcalloc((size_t)(nt > 0 ? nt : 1), sizeof(uint64_t)); }
static void cov_push(covlist* c, covseg sg)
{
    if (c->n == c->cap) { c->cap = c->cap ? c->cap * 2 : 64; c->seg = xrealloc(c->seg, sizeof(covseg) * (size_t)c->cap); }
    c->seg[c->n++] = sg;
}
static void cov_close(covlist* c) { if (c->open) { cov_push(c, c->cur); c->open = 0; } }
static void cov_free(covlist* c) { free(c->sum); free(c->seg); memset(c, 0, sizeof *c); }
static inline void cov_record(covlist* c, const bam_record* b)
{
    if (b->flag & (0x4 | 0x100 | 0x200 | 0x400)) return;
    if (b->tid < 0 || b->tid >= c->nt || b->pos < 0) return;
    const int32_t end = bam_record_end(b);
    if (end <= b->pos) return;                                  /* no reference base: the pileup drops it unseen */
    c->sum[b->tid] += (uint64_t)(end - b->pos);
    if (c->open && c->cur.tid == b->tid && b->pos >= c->cur.beg && b->pos <= c->cur.end) { if (end > c->cur.end) c->cur.end = end; return; }
    cov_close(c);
    c->cur.tid = b->tid; c->cur.beg = b->pos; c->cur.end = end; c->open = 1;
}
static int cmp_covseg(const void* x, const void* y)
{
    const covseg* a = x; const covseg* b = y;
    if (a->tid != b->tid) return a->tid < b->tid ? -1 : 1;
    if (a->beg != b->beg) return a->beg < b->beg ? -1 : 1;
    return 0;
}
/* sums[nt] and the segments of every walker -> g_meancov */
static void cov_means(int32_t nt, const uint64_t* sums, covseg* seg, int64_t n)
{
    if (!g_meancov) g_meancov = xcalloc((size_t)(nt > 0 ? nt : 1), sizeof(uint32_t));
    uint64_t* covered = xcalloc((size_t)(nt > 0 ? nt : 1), sizeof(uint64_t));
    qsort(seg, (size_t)n, sizeof(covseg), cmp_covseg);
    for (int64_t i = 0; i < n; ) {
        const int32_t t = seg[i].tid;
        int32_t beg = seg[i].beg, end = seg[i].end;
        for (i++; i < n && seg[i].tid == t && seg[i].beg <= end; i++) if (seg[i].end > end) end = seg[i].end;
        covered[t] += (uint64_t)(end - beg);
    }
    for (int32_t t = 0; t < nt; t++) if (covered[t]) g_meancov[t] = (uint32_t)floor((double)sums[t] * 1.0 / (double)covered[t]);
    free(covered);
}
static void cov_means_of_lists(int32_t nt, covlist* const* ls, int n_lists)
{
    uint64_t* sums = xcalloc((size_t)(nt > 0 ? nt : 1), sizeof(uint64_t));
    int64_t n = 0;
    for (int i = 0; i < n_lists; i++) { cov_close(ls[i]); n += ls[i]->n; }
    covseg* seg = xmalloc(sizeof(covseg) * (size_t)(n ? n : 1));
    n = 0;
    for (int i = 0; i < n_lists; i++) {
        for (int32_t t = 0; t < nt; t++) sums[t] += ls[i]->sum[t];
        if (ls[i]->n) memcpy(seg + n, ls[i]->seg, sizeof(covseg) * (size_t)ls[i]->n);
        n += ls[i]->n;
    }
    cov_means(nt, sums, seg, n);
    free(sums); free(seg);
}
static void cov_print_table(const bam_header* hdr)
{
    /* src/indelminer.c:728-733 */
    fprintf(stderr, "\nChromosomeID\tMean-coverage\n-------------\t-----------\n");
    for (int32_t i = 0; i < hdr->n_targets; i++) fprintf(stderr, "%d\t%u\n", i, g_meancov ? g_meancov[i] : 0u);
    fprintf(stderr, "-------------\t-----------\n\n");
}

static void estimate_insertlengths(driver* d, int chromid)
{
    /* src/bamoperations.c:15-86: min / max proper-pair isize per read group */
    bgzf_reader* r = bgzf_open(d->bam_name);
    if (!r) fatalf("error in opening the file %s", d->bam_name);
    bam_header* h = bam_header_load(r);
    bam_record b; memset(&b, 0, sizeof b);
    covlist cov;
    cov_init(&cov, h->n_targets);
    for (int32_t t = 0; t < h->n_targets; t++) {
        if (chromid != -1 && t != chromid) continue;
        bam_region_iter it;
        if (bam_region_begin(&it, r, d->idx, t, 0, h->target_len[t]) != 0) continue;
        while (bam_region_next(&it, &b) == 1) {
            cov_record(&cov, &b);
            if ((b.flag & 0x1) == 0 || (b.flag & 0x4) || (b.flag & 0x2) == 0) continue;
            if (b.flag & (0x100 | 0x200 | 0x400)) continue;
            if (b.isize < 0) continue;
            const uint8_t* rg = bam_aux_find(&b, "RG");
            const char* rgname = "generic";
            if (rg) { forceassert(rg[0] == 'Z'); rgname = bam_aux_str(rg); }
            const int32_t isize = b.isize;
            if (b.mpos - b.pos < 0) continue;
            if (isize < b.mpos - b.pos) continue;
            qbin* q = qhash_lookup(d->insertlengths, rgname, (int)strlen(rgname));
            if (!q) {
                int32_t* range = xmalloc(2 * sizeof(int32_t));
                range[0] = range[1] = isize;
                qhash_add(d->insertlengths, rgname, (int)strlen(rgname), range);
                rg_order_push(rgname, range);
            } else {
                int32_t* range = q->val;
                if (range[0] > isize) range[0] = isize;
                if (range[1] < isize) range[1] = isize;
            }
        }
    }
    free(b.data);
    { covlist* one = &cov; cov_means_of_lists(h->n_targets, &one, 1); cov_free(&cov); }
    bam_header_free(h);
    bgzf_close(r);
}

/* --------------------------------------------------------------- preamble -- */

static void print_vcf_preamble(void)
{
    /* src/shared.c:84-109, byte for byte */
    printf("##fileformat=VCFv4.1\n");
    printf("##%sVersion=%2.2f\n", "indelminer", INDELMINER_VERSION);
    printf("##INFO=<ID=INSERTION,Number=0,Type=Flag,Description=\"Indicates that the variant is an insertion.\">\n");
    printf("##INFO=<ID=DELETION,Number=0,Type=Flag,Description=\"Indicates that the variant is a deletion.\">\n");
    printf("##INFO=<ID=SPLIT_READ,Number=0,Type=Flag,Description=\"Indicates that at least one split read supports this variant.\">\n");
    printf("##INFO=<ID=PAIRED_READ,Number=0,Type=Flag,Description=\"Indicates that at least one PE read supports this variant.\">\n");
    printf("##INFO=<ID=COMPOSITE,Number=0,Type=Flag,Description=\"Indicates that at least one split read and at least one PE read supports this variant.\">\n");
    printf("##INFO=<ID=NS,Number=1,Type=Integer,Description=\"Number of reads supporting the variant\">\n");
    printf("##INFO=<ID=END,Number=1,Type=Integer,Description=\"end position of the variant described in this record\">\n");
    printf("##INFO=<ID=BP_END,Number=1,Type=Integer,Description=\"possible 3' end of the breakpoint described in this record\">\n");
    printf("##INFO=<ID=NFS,Number=1,Type=Integer,Description=\"Number of reads supporting the variant on the forward strand\">\n");
    printf("##INFO=<ID=NRS,Number=1,Type=Integer,Description=\"Number of reads supporting the variant on the forward strand\">\n");
    printf("##INFO=<ID=UTAILS,Number=1,Type=Integer,Description=\"The number of unique tail distances in supporting reads for this variant\">\n");
    printf("##INFO=<ID=MQ,Number=1,Type=Integer,Description=\"RMS mapping quality of the reads covering the breakpoints\">\n");
    printf("##INFO=<ID=MQ30,Number=1,Type=Integer,Description=\"Number of reads with mapping quality greater than or equal to 30, covering the breakpoints\">\n");
    printf("##INFO=<ID=DF,Number=1,Type=Integer,Description=\"Average number of other differences on reads supporting the reported variant\">\n");
    printf("##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Average read depth across the breakpoints\">\n");
    printf("##INFO=<ID=BF,Number=2,Type=Integer,Description=\"Flanks from the split read or pair best sorrounding the variant\">\n");
}

/* ----------------------------------------------------------------- pass B -- */

/* the evidence one candidate read contributes: the realigned segments when the GPU found any
 * (they replace the CIGAR-derived ones, src/indelminer.c:494-502), else the CIGAR-derived */
static void resolve_candidate(driver* d, const item_t* it, const im_read_result* r, int32_t tid)
{
    const cand_batch* cb = &d->cb;
    const int c = it->cand;
    if (r->status == IM_ST_EVIDENCE && r->n_ev > 0) {
        seglist whole;
        whole.ref_start = r->ref_start; whole.n = r->n_ops;
        whole.ops = (uint32_t*)r->ops;
        const int64_t len = cb->base_off[c + 1] - cb->base_off[c];
        char* bases = xmalloc((size_t)len + 1);
        memcpy(bases, cb->bases + cb->base_off[c], (size_t)len); bases[len] = 0;
        whole.bases = bases;
        for (int k = 0; k < r->n_ev; k++) {
            const im_evidence* ge = &r->ev[k];
            evidence_t* e = xcalloc(1, sizeof *e);
            e->type = EV_SPLIT_READ; e->cls = ge->cls; e->strand = cb->strand[c]; e->qual = cb->qual[c];
            e->qname = xstrdup(cb->qname[c]);
            e->aln = seglist_copy(&whole);
            e->seg = ge->seg; e->b1 = ge->b1; e->b2 = ge->b2;
            e->lflank = ge->lflank; e->rflank = ge->rflank; e->nd_print = ge->nd_print; e->nd_filter = ge->nd_filter;
            pending_push(d, e);
        }
        free(bases);
        for (int k = 0; k < it->nbwa; k++) evidence_free(it->bwa[k]);
    } else {
        for (int k = 0; k < it->nbwa; k++) pending_push(d, it->bwa[k]);
    }
    (void)tid;
}

static void ivl_push(ivlist* l, int32_t start, int32_t len)
{
    if (l->n == l->cap) {
        l->cap = l->cap ? l->cap * 2 : (1 << 16);
        l->start = xrealloc(l->start, sizeof(int32_t) * (size_t)l->cap);
        l->len = xrealloc(l->len, sizeof(int32_t) * (size_t)l->cap);
    }
    l->start[l->n] = start; l->len[l->n] = len; l->n++;
}

/* the size of -V's table: the smallest 2^k >= max(65 536, BAM bytes / 64), at most 2^30 (DESIGN.md 4.5f has the reasoning) */
static int evidence_table_log2(const driver* d)
{
    struct stat sb;
    const int64_t bytes = stat(d->bam_name, &sb) == 0 ? (int64_t)sb.st_size : 0;
    int k = 16;
    while (k < 30 && ((int64_t)1 << k) < bytes / 64) k++;
    return k;
}

#define GPU2(drv, call) do { if ((call) != IM_OK) fatalf("%s: %s", #call, im_last_error((drv)->gpu)); } while (0)
#define EVIDENCE_ON (SPAN_ON || PAIR_ON || CLIP_ON || PAIRTABLE_ON || MATETABLE_ON || SPLITTABLE_ON)     /* -V needs -C */

/* Once per run, on either path, when the reference is on the device and the insert lengths are known: what the evidence options
 * keep on the device.  Genome-wide arrays and tables keyed by contig: nothing is reset between contigs. */
static void evidence_enable(driver* d)
{
    /* the insert-length table in the order its entries were added, range[1] of each */
    int32_t* rmax = xmalloc(sizeof(int32_t) * (size_t)(g_rg_n ? g_rg_n : 1));
    for (int i = 0; i < g_rg_n; i++) rmax[i] = g_rg_range[i][1];
    GPU2(d, im_set_insert_ranges(d->gpu, g_rg_n, g_rg_name, rmax));
    free(rmax);
    /* -G: the second genome-wide array, only then */
    if (SPAN_ON) GPU2(d, im_span_enable(d->gpu, (int32_t)O.ethreshold, O.qthreshold));
    /* -P: and a third */
    if (PAIR_ON) GPU2(d, im_pairspan_enable(d->gpu, (int32_t)O.ethreshold, O.qthreshold));
    /* -C: and the two arrays of clipped-read counts */
    if (CLIP_ON) GPU2(d, im_clip_enable(d->gpu, CLIP_EV_MIN_CLIP, O.qthreshold));
    /* -V: and the table of their clipped bases */
    if (CLIPTAIL_ON) GPU2(d, im_cliptail_enable(d->gpu, CLIP_EV_MIN_CLIP, O.qthreshold, evidence_table_log2(d)));
    /* -M: and the table of pair links, -V's rule with one sixteenth of its slots (LINK_EV_SLOTS_SHIFT says what that assumes) */
    if (PAIRTABLE_ON) GPU2(d, im_pairlink_enable(d->gpu, O.qthreshold, evidence_table_log2(d) - LINK_EV_SLOTS_SHIFT));
    /* -E: with its fourth kind, the stretched pairs, in front of the first scatter */
    if (JUNCPAIR_ON) GPU2(d, im_pairlink_stretched_enable(d->gpu));
    /* -T: and the table of mate links, of the same size on the same assumption, which nobody has measured here either */
    if (MATETABLE_ON) GPU2(d, im_matelink_enable(d->gpu, O.qthreshold, evidence_table_log2(d) - LINK_EV_SLOTS_SHIFT));
    /* -S, -J: and the table of split links, -C's clip and -q, the contig names as the BAM header spells them, in tid order; the same size
     * on an assumption of its own (SPLIT_EV_SLOTS_SHIFT), which nobody has measured either */
    if (SPLITTABLE_ON) GPU2(d, im_splitlink_enable(d->gpu, CLIP_EV_MIN_CLIP, O.qthreshold, evidence_table_log2(d) - SPLIT_EV_SLOTS_SHIFT, d->hdr->n_targets,
                                                  (const char* const*)d->hdr->target_name));
    /* -H: and the overlap array beside it, two bytes per slot, in front of the first scatter */
    if (JUNCOVL_ON) GPU2(d, im_splitlink_overlap_enable(d->gpu));
}

/* a chunk of records on the device, as they are in the file: each option's record rule is its scatter kernel's, on either path */
static void evidence_scatter(driver* d, const im_dev_records* recs, void* stream)
{
    if (SPAN_ON) GPU2(d, im_dev_span_scatter(d->gpu, recs, stream));            /* -G, -A */
    if (PAIR_ON) GPU2(d, im_dev_pairspan_scatter(d->gpu, recs, stream));        /* -P: one more, only then */
    if (CLIP_ON) GPU2(d, im_dev_clip_scatter(d->gpu, recs, stream));            /* -C: one more, only then; these arrays need no scan */
    if (CLIPTAIL_ON) GPU2(d, im_dev_cliptail_scatter(d->gpu, recs, stream));    /* -V: and one behind it, only then */
    if (PAIRTABLE_ON) GPU2(d, im_dev_pairlink_scatter(d->gpu, recs, stream));   /* -M, -E: and one behind that, only then */
    if (MATETABLE_ON) GPU2(d, im_dev_matelink_scatter(d->gpu, recs, stream));   /* -T, -E: and one behind that, only then */
    if (SPLITTABLE_ON) GPU2(d, im_dev_splitlink_scatter(d->gpu, recs, stream)); /* -S, -J: and one behind that, only then */
}

/* The chunks of both paths: the pipelined walk's ring has up to PIPE_NCHUNK of them per walker (host_pipeline.c), the record-at-a-time
 * path cycles one. */
static uint32_t g_chunk_bytes = 32u << 20;
#define PIPE_CHUNK_BYTES   g_chunk_bytes
#define PIPE_CHUNK_RECS    (g_chunk_bytes / 64u)

/* The record-at-a-time path's chunk.  Pass A reads its records into one host buffer, 4-byte aligned and zero padded like the walk's;
 * with an evidence option on, the buffer goes to a device twin and through the scatters whenever it is full, holds its cap of records,
 * or the pass ends.  Nothing overlaps: every submit ends synchronised, so the queries that follow on the context's stream see it.
 * INDELMINER_HOST_CHUNK_RECS lowers the cap (tests: a cap that cuts inside the scatters' workgroups). */
static void host_chunk_submit(driver* d)
{
    if (d->ck_n > 0 && EVIDENCE_ON) {
        void* stream = im_ctx_stream(d->gpu);
        d->ck_off[d->ck_n] = d->ck_bytes;
        GPU2(d, im_dev_upload_async(d->gpu, d->ck_draw, d->ck_raw, d->ck_bytes, stream));
        GPU2(d, im_dev_upload_async(d->gpu, d->ck_doff, d->ck_off, 4 * ((size_t)d->ck_n + 1), stream));
        im_dev_records recs = { d->ck_n, d->ck_draw, d->ck_doff, 0 };
        evidence_scatter(d, &recs, stream);
        GPU2(d, im_stream_sync(d->gpu, stream));
    }
    d->ck_n = 0; d->ck_bytes = 0;
}

static void host_chunk_init(driver* d)
{
    if (d->ck_raw) return;
    const char* e = getenv("INDELMINER_HOST_CHUNK_RECS");
    d->ck_cap = (int32_t)PIPE_CHUNK_RECS;
    if (e && atoi(e) >= 1 && atoi(e) < d->ck_cap) d->ck_cap = atoi(e);
    d->ck_raw = xmalloc(PIPE_CHUNK_BYTES);
    d->ck_off = xmalloc(4 * ((size_t)d->ck_cap + 1));
    if (!EVIDENCE_ON) return;
    GPU2(d, im_dev_alloc(d->gpu, (size_t)PIPE_CHUNK_BYTES + 64, &d->ck_draw));     /* the kernels read up to 64 bytes past the last record */
    GPU2(d, im_dev_alloc(d->gpu, 4 * ((size_t)d->ck_cap + 1), &d->ck_doff));
}

/* the next record of the pass into the chunk (submitting what it holds when that is what makes room): 1 and the view, or 0 at the end */
static int host_chunk_next(driver* d, bam_region_iter* it, bam_record* b)
{
    for (;;) {
        int32_t len = 0;
        const int rc = d->ck_n < d->ck_cap ? bam_region_next_raw(it, d->ck_raw + d->ck_bytes, (int64_t)PIPE_CHUNK_BYTES - d->ck_bytes, &len, b) : -2;
        if (rc == -2) {
            if (d->ck_n == 0) fatalf("a BAM record larger than %u bytes", PIPE_CHUNK_BYTES);
            host_chunk_submit(d);
            continue;
        }
        if (rc != 1) return 0;
        d->ck_off[d->ck_n++] = d->ck_bytes;
        for (uint32_t z = (uint32_t)len; z & 3u; z++) d->ck_raw[d->ck_bytes + z] = 0;
        d->ck_bytes += ((uint32_t)len + 3u) & ~3u;
        return 1;
    }
}

/* An evidence FILE (-I, -U, -N): opened when its first contig is about to be searched (a run handed to the record-at-a-time child
 * never gets here in the parent: the child writes the file), finished when the last has been -- or with the header alone. */
typedef struct evfile {
    const char* const* path; FILE* out;                 /* the option's argument (NULL: not given), the file once it is open */
    void (*describe)(FILE* f);                          /* the ##ALT, ##INFO and description lines */
    void (*contig)(driver* d, int32_t tid, FILE* f);    /* one contig's records */
    const char* phase;
} evfile;

static FILE* ev_open(evfile* e)
{
    if (e->out) return e->out;
    e->out = fopen(*e->path, "w");
    if (!e->out) fatalf("cannot write %s", *e->path);
    fprintf(e->out, "##fileformat=VCFv4.1\n");
    e->describe(e->out);
    fprintf(e->out, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n");
    return e->out;
}

/* one contig, whose every record the clip arrays and the tables hold: behind the last flush (pipelined) or the contig's (record-at-a-time) */
static void ev_contig(evfile* e, driver* d, int32_t tid)
{
    FILE* f = ev_open(e);
    gpu_wait(d);
    e->contig(d, tid, f);
    phase_time(e->phase);
}

static void ev_finish(evfile* e)
{
    if (fclose(ev_open(e)) != 0) fatalf("cannot write %s", *e->path);     /* no contig at all: the header alone */
    e->out = NULL;
}

static void ins_describe(FILE* f)
{
    fprintf(f, "##ALT=<ID=INS,Description=\"Insertion too long for a read to span: clipped reads from either side face each other\">\n");
    fprintf(f, "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n");
    fprintf(f, "##INFO=<ID=END,Number=1,Type=Integer,Description=\"Where the reads from the left stop aligning (POS: where the reads from the right start)\">\n");
    fprintf(f, "##INFO=<ID=HOMLEN,Number=1,Type=Integer,Description=\"END - POS: bases aligned from both sides (target-site duplication or micro-homology)\">\n");
    fprintf(f, "##INFO=<ID=CR,Number=2,Type=Integer,Description=\"Clipped reads that stop aligning at END, clipped reads that start aligning at POS\">\n");
    fprintf(f, "##INFO=<ID=CN,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases were kept, either side\">\n");
    fprintf(f, "##INFO=<ID=CA,Number=2,Type=Integer,Description=\"Of those, the reads that agree with the consensus of their side\">\n");
    fprintf(f, "##INFO=<ID=LSEQ,Number=1,Type=String,Description=\"First bases of the inserted sequence: consensus of the clipped bases behind END\">\n");
    fprintf(f, "##INFO=<ID=RSEQ,Number=1,Type=String,Description=\"Last bases of the inserted sequence: consensus of the clipped bases in front of POS\">\n");
    fprintf(f, "##largeInsertion=\"a record per position END at which at least %d reads of mapping quality >= -q stop aligning with a soft clip of at least %d bases, "
               "more than at any of the %d positions in front and no fewer than at any of the %d behind, when at least %d such reads start aligning at one of "
               "the positions END - %d .. END (POS: the one with the most, the nearest to END among equals); LSEQ and RSEQ: per base the majority of up to 32 "
               "clipped bases per read (A before C before G before T among equals), as far as at least %d reads reach; CA: reads with at most 1 difference "
               "in 16 from it; CN, CA, LSEQ and RSEQ are . once the clip-tail table has overflowed (stderr says so); contig ends are skipped\"\n",
            INS_EV_MIN_READS, CLIP_EV_MIN_CLIP, INS_EV_MAX_OVERLAP, INS_EV_MAX_OVERLAP, INS_EV_MIN_READS, INS_EV_MAX_OVERLAP, INS_EV_MIN_COVER);
}

/* the consensus of one pile as text: base 0 first, or (the left pile, turned back to reference orientation) base len - 1 first */
static void ins_seq(char* out, uint32_t len, uint32_t lo, uint32_t hi, int reversed)
{
    if (len == 0 || len > CLIPTAIL_BASES) { strcpy(out, "."); return; }
    for (uint32_t i = 0; i < len; i++) {
        const uint32_t k = reversed ? len - 1 - i : i;
        out[i] = "ACGT"[((lo >> k) & 1u) | (((hi >> k) & 1u) << 1)];
    }
    out[len] = 0;
}

/* -I: one contig's facing piles and the consensus of either pile, into FILE */
static void ins_contig(driver* d, int32_t tid, FILE* f)
{
    const int64_t clen = d->seqlen[tid];
    int32_t cap = 65536, found = 0;
    int32_t* pr = NULL; int32_t* pl = NULL; uint32_t* cr = NULL; uint32_t* cl = NULL;
    pthread_mutex_lock(&g_query_mu);
    for (;;) {
        pr = xrealloc(pr, sizeof(int32_t) * (size_t)cap); pl = xrealloc(pl, sizeof(int32_t) * (size_t)cap);
        cr = xrealloc(cr, sizeof(uint32_t) * (size_t)cap); cl = xrealloc(cl, sizeof(uint32_t) * (size_t)cap);
        const int rc = im_clip_facing_tid(d->gpu, tid, INS_EV_MIN_READS, INS_EV_MAX_OVERLAP, cap, pr, pl, cr, cl, &found);
        if (rc != IM_OK) fatalf("im_clip_facing: %s", im_last_error(d->gpu));
        if (found <= cap) break;
        cap = found;                /* more piles than asked for: once more, with room for all */
    }
    /* contig ends have nothing to anchor on */
    int32_t n = 0;
    for (int32_t k = 0; k < found; k++)
        if (pl[k] != 0 && pr[k] != clen) { pr[n] = pr[k]; pl[n] = pl[k]; cr[n] = cr[k]; cl[n] = cl[k]; n++; }
    if (n > 0) {
        /* two queries per pile: right at pr, left at pl */
        int32_t* qpos = xmalloc(sizeof(int32_t) * 2 * (size_t)n);
        uint8_t* qside = xmalloc(2 * (size_t)n);
        uint32_t* ans = xmalloc(sizeof(uint32_t) * 10 * (size_t)n);
        uint32_t* ent = ans; uint32_t* len = ans + 2 * n; uint32_t* agree = ans + 4 * n; uint32_t* planes = ans + 6 * n;
        for (int32_t k = 0; k < n; k++) { qpos[2 * k] = pr[k]; qside[2 * k] = 0; qpos[2 * k + 1] = pl[k]; qside[2 * k + 1] = 1; }
        if (im_cliptail_consensus(d->gpu, tid, 2 * n, qpos, qside, INS_EV_MIN_COVER, ent, len, planes, agree) != IM_OK)
            fatalf("im_cliptail_consensus: %s", im_last_error(d->gpu));
        const char* seq = d->sequences[tid];
        for (int32_t k = 0; k < n; k++) {
            fprintf(f, "%s\t%d\t.\t%c\t<INS>\t.\t.\tSVTYPE=INS;END=%d;HOMLEN=%d;CR=%u,%u;", d->hdr->target_name[tid], pl[k],
                    toupper((unsigned char)seq[pl[k] - 1]), pr[k], pr[k] - pl[k], cr[k], cl[k]);
            if (ent[2 * k] == CLIPTAIL_NONE) { fprintf(f, "CN=.;CA=.;LSEQ=.;RSEQ=.\n"); continue; }
            char ls[CLIPTAIL_BASES + 1], rs[CLIPTAIL_BASES + 1];
            ins_seq(ls, len[2 * k], planes[4 * k], planes[4 * k + 1], 0);
            ins_seq(rs, len[2 * k + 1], planes[4 * k + 2], planes[4 * k + 3], 1);
            fprintf(f, "CN=%u,%u;CA=%u,%u;LSEQ=%s;RSEQ=%s\n", ent[2 * k], ent[2 * k + 1], agree[2 * k], agree[2 * k + 1], ls, rs);
        }
        free(qpos); free(qside); free(ans);
    }
    pthread_mutex_unlock(&g_query_mu);
    free(pr); free(pl); free(cr); free(cl);
}

/* -M: the ##pairLinks line, the rule and its constants (the ##INFO line of PE is the FILE's own: dup_describe, inv_describe) */
static void pe_describe(FILE* f)
{
    fprintf(f, "##pairLinks=\"PE counts read pairs on one contig, each once at its leftmost read: paired, both reads mapped, neither secondary, supplementary, duplicate "
               "nor failing quality control, the leftmost read of mapping quality >= -q, both starts inside the contig, in the orientation of the record's junction "
               "(the normal one, forward in front of reverse, never counts, whatever its insert size); start of the leftmost read and start of its mate each within a "
               "window that reaches %d bases from the record's breakpoint towards where the junction's pairs lie and %d bases the other way, the two starts at "
               "least %d bases apart; PE is . once the pair-link table has overflowed (stderr says so); a duplication shorter than a read leaves no everted pair: "
               "PE=0 is expected there; pairs whose mate lies on another contig are not counted\"\n", LINK_EV_WINDOW, CLIPTAIL_MAX_SHIFT, LINK_EV_MIN_SEP);
}

/* -M: PE of one contig's records, one query each; kind, and the two windows [a0, a1] (pos) and [b0, b1] (mpos) as the caller filled them.
 * The device clips the windows to the contig; what an int32 does not hold is clipped here. */
static int32_t link_clamp(int64_t x) { return (int32_t)(x < INT32_MIN ? INT32_MIN : x > INT32_MAX ? INT32_MAX : x); }
static uint32_t* pair_links_query(driver* d, int32_t tid, int32_t n, const uint8_t* kind, const int32_t* win)
{
    uint32_t* pe = xmalloc(sizeof(uint32_t) * (size_t)(n > 0 ? n : 1));
    pthread_mutex_lock(&g_query_mu);
    const int rc = im_pairlink_count(d->gpu, tid, n, kind, win, win + n, win + 2 * (size_t)n, win + 3 * (size_t)n, LINK_EV_MIN_SEP, pe);
    pthread_mutex_unlock(&g_query_mu);
    if (rc != IM_OK) fatalf("im_pairlink_count: %s", im_last_error(d->gpu));
    return pe;
}
static void fprint_pe(FILE* f, uint32_t pe)
{
    if (pe == PAIRLINK_NONE) fprintf(f, ";PE=."); else fprintf(f, ";PE=%u", pe);
}

/* -S: the ##INFO line of SR and the ##splitLinks line, the rule and its constants, the same in the three FILEs */
static void sr_info(FILE* f)
{
    fprintf(f, "##INFO=<ID=SR,Number=2,Type=Integer,Description=\"Split reads whose primary part is clipped within %d bases of the record's first breakpoint and whose SA tag "
               "places the clipped part within %d bases of its second breakpoint, and the same from the second to the first\">\n", SPLIT_EV_WINDOW, SPLIT_EV_WINDOW);
}
static void sr_describe(FILE* f)
{
    fprintf(f, "##splitLinks=\"SR counts primary records (neither unmapped, secondary, supplementary, duplicate nor failing quality control; paired or not) of mapping "
               "quality >= -q with a soft clip of at least %d bases on the side of the breakpoint whose SA tag holds exactly one entry, of mapping quality >= -q, "
               "inside the contig it names, that places the clipped part of the read: the primary part ends at one breakpoint of the record, on the side the "
               "record's pile is clipped on, and the other part ends at the other, both within %d bases; the first number counts the reads whose primary record "
               "lies at the record's first breakpoint, the second those at its second; a tag with several entries is not counted; SR is . once the split-link "
               "table has overflowed (stderr says so)\"\n", CLIP_EV_MIN_CLIP, SPLIT_EV_WINDOW);
}

/* -S: SR of n records, two queries each: from the first end (tid1, p1, side1) to the second (tid2, p2, side2), and back; windows of
 * SPLIT_EV_WINDOW bases around either position (the device clips them to the contig; what an int32 does not hold is clipped here).
 * sr[k], sr[n + k]: the two counts of record k. */
static uint32_t* split_links_query(driver* d, int32_t n, const int32_t* tid1, const int32_t* p1, const uint8_t* side1, const int32_t* tid2, const int32_t* p2,
                                   const uint8_t* side2)
{
    const size_t m = 2 * (size_t)(n > 0 ? n : 1);
    uint32_t* sr = xmalloc(sizeof(uint32_t) * m);
    int32_t* q = xmalloc(sizeof(int32_t) * 6 * m); uint8_t* qs = xmalloc(2 * m);
    int32_t* ta = q; int32_t* a0 = q + m; int32_t* a1 = q + 2 * m; int32_t* tb = q + 3 * m; int32_t* b0 = q + 4 * m; int32_t* b1 = q + 5 * m;
    for (int32_t k = 0; k < 2 * n; k++) {
        const int back = k >= n;
        const int32_t j = k % n;
        const int64_t pa = back ? p2[j] : p1[j], pb = back ? p1[j] : p2[j];
        ta[k] = back ? tid2[j] : tid1[j]; tb[k] = back ? tid1[j] : tid2[j];
        qs[k] = back ? side2[j] : side1[j]; qs[m + k] = back ? side1[j] : side2[j];
        a0[k] = link_clamp(pa - SPLIT_EV_WINDOW); a1[k] = link_clamp(pa + SPLIT_EV_WINDOW);
        b0[k] = link_clamp(pb - SPLIT_EV_WINDOW); b1[k] = link_clamp(pb + SPLIT_EV_WINDOW);
    }
    pthread_mutex_lock(&g_query_mu);
    const int rc = im_splitlink_count(d->gpu, 2 * n, ta, qs, a0, a1, tb, qs + m, b0, b1, sr);
    pthread_mutex_unlock(&g_query_mu);
    if (rc != IM_OK) fatalf("im_splitlink_count: %s", im_last_error(d->gpu));
    free(q); free(qs);
    return sr;
}
static void fprint_sr(FILE* f, uint32_t n1, uint32_t n2)
{
    if (n1 == SPLITLINK_NONE) fprintf(f, ";SR=."); else fprintf(f, ";SR=%u,%u", n1, n2);
}
/* the same for the pile pairs of one contig: the ends' positions are columns a and b of pos, the sides s1 and s2 (side: per pair, or null) */
static uint32_t* split_links_pairs(driver* d, int32_t tid, int32_t n, const int32_t* pa, const int32_t* pb, const uint8_t* side, uint8_t s1, uint8_t s2)
{
    int32_t* t = xmalloc(sizeof(int32_t) * (size_t)n); uint8_t* s = xmalloc(2 * (size_t)n);
    for (int32_t k = 0; k < n; k++) { t[k] = tid; s[k] = side ? side[k] : s1; s[n + k] = side ? side[k] : s2; }
    uint32_t* sr = split_links_query(d, n, t, pa, s, t, pb, s + n);
    free(t); free(s);
    return sr;
}

static void dup_describe(FILE* f)
{
    fprintf(f, "##ALT=<ID=DUP:TANDEM,Description=\"Tandem duplication: reads clipped at its end continue at its start\">\n");
    fprintf(f, "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n");
    fprintf(f, "##INFO=<ID=END,Number=1,Type=Integer,Description=\"Last duplicated base: where the reads from the left stop aligning (POS + 1: the first, where the reads from the right start)\">\n");
    fprintf(f, "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"END - POS: bases duplicated\">\n");
    fprintf(f, "##INFO=<ID=HOMLEN,Number=1,Type=Integer,Description=\"Bases by which the clipped reads continue behind the other breakpoint (micro-homology the aligner extended into)\">\n");
    fprintf(f, "##INFO=<ID=CR,Number=2,Type=Integer,Description=\"Clipped reads that stop aligning at END, clipped reads that start aligning at POS\">\n");
    fprintf(f, "##INFO=<ID=CN,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases were kept, either side\">\n");
    fprintf(f, "##INFO=<ID=CV,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases are the reference at the other breakpoint\">\n");
    if (g_depth_evidence) {
        fprintf(f, "##INFO=<ID=DM,Number=3,Type=Integer,Description=\"Median depth over the duplicated bases POS+1..END, over the %d bases in front of them and over the %d bases behind them\">\n", DEPTH_EV_FLANK, DEPTH_EV_FLANK);
        fprintf(f, "##INFO=<ID=DFC,Number=1,Type=Integer,Description=\"Depth fold change in thousandths: the first DM value over the mean of the other two\">\n");
    }
    if (PAIRLINK_ON)
        fprintf(f, "##INFO=<ID=PE,Number=1,Type=Integer,Description=\"everted read pairs (the leftmost read reverse, its mate forward) that start within POS - %d .. POS + %d "
                   "and whose mate starts within END - %d .. END + %d, at least %d bases apart\">\n", CLIPTAIL_MAX_SHIFT, LINK_EV_WINDOW, LINK_EV_WINDOW, CLIPTAIL_MAX_SHIFT, LINK_EV_MIN_SEP);
    if (SPLITLINK_ON) sr_info(f);
    fprintf(f, "##tandemDuplication=\"a record per pair of positions END and POS, %d <= END - POS <= %d, where END is a position at which at least %d reads of mapping "
               "quality >= -q stop aligning with a soft clip of at least %d bases, more than at any of the %d positions in front and no fewer than at any of the %d "
               "behind, and POS is such a position of the reads that start aligning with such a clip, when for one shift s in 0 .. %d at least %d of the reads at END "
               "continue with the reference from POS + s on and at least %d of the reads at POS continue backwards with the reference from END - 1 - s on, in up to 32 "
               "clipped bases per read with at most 1 difference in 16 (HOMLEN: the s with the most such reads, the smallest among equals; CV: those reads); "
               "the file has no records once the clip-tail table has overflowed (stderr says so); POS 0 is skipped\"\n",
            DUP_EV_MIN_LEN, DUP_EV_MAX_LEN, DUP_EV_MIN_READS, CLIP_EV_MIN_CLIP, DUP_EV_REACH, DUP_EV_REACH, CLIPTAIL_MAX_SHIFT, DUP_EV_MIN_VERIFIED, DUP_EV_MIN_VERIFIED);
    if (PAIRLINK_ON) pe_describe(f);
    if (SPLITLINK_ON) sr_describe(f);
}

/* The pairs of piles of one contig, crossed (-U) or inverted (-N).  Columns of cap: pos = p1 p2 shift | cnt = c1 c2 v1 v2 stored at p1,
 * stored at p2 | side (inverted alone).  found < 0: the table has overflowed, the header alone. */
typedef struct pile_pairs { int32_t cap, found; int32_t* pos; uint32_t* cnt; uint8_t* side; } pile_pairs;

static pile_pairs pile_pairs_query(driver* d, int32_t tid, int inverted)
{
    pile_pairs P = {4096, 0, NULL, NULL, NULL};
    pthread_mutex_lock(&g_query_mu);
    for (;; P.cap = P.found) {      /* more pairs than asked for: once more, with room for all */
        const int32_t cap = P.cap;
        int32_t* pos = P.pos = xrealloc(P.pos, sizeof(int32_t) * 3 * (size_t)cap);
        uint32_t* cnt = P.cnt = xrealloc(P.cnt, sizeof(uint32_t) * 6 * (size_t)cap);
        if (inverted) P.side = xrealloc(P.side, (size_t)cap);
        const int rc = inverted
            ? im_clip_inverted_tid(d->gpu, tid, INV_EV_MIN_READS, INV_EV_REACH, INV_EV_MIN_LEN, INV_EV_MAX_LEN, CLIPTAIL_MAX_SHIFT,
                  INV_EV_MIN_VERIFIED, cap, P.side, pos, pos + cap, cnt, cnt + cap, cnt + 2 * cap, cnt + 3 * cap, pos + 2 * cap, cnt + 4 * cap, cnt + 5 * cap, &P.found)
            : im_clip_crossed_tid(d->gpu, tid, DUP_EV_MIN_READS, DUP_EV_REACH, DUP_EV_MIN_LEN, DUP_EV_MAX_LEN, CLIPTAIL_MAX_SHIFT,
                  DUP_EV_MIN_VERIFIED, cap, pos, pos + cap, cnt, cnt + cap, cnt + 2 * cap, cnt + 3 * cap, pos + 2 * cap, cnt + 4 * cap, cnt + 5 * cap, &P.found);
        if (rc != IM_OK) fatalf("%s: %s", inverted ? "im_clip_inverted" : "im_clip_crossed", im_last_error(d->gpu));
        if (P.found <= cap) break;
    }
    pthread_mutex_unlock(&g_query_mu);
    return P;
}

/* -U: one contig's crossed piles into FILE.  With -D the contig's scanned depth array is resident as well -- the genome-wide array is
 * scanned contig by contig as the walk leaves each (im_depth_scan) and never reset; the record-at-a-time path has built this contig's
 * depth array alone (im_depth_build) and scattered the rest like the walk.
 * g_query_mu is taken again for the depth queries: the pairs are on the host by then, so nothing needs it held in between. */
static void dup_contig(driver* d, int32_t tid, FILE* f)
{
    pile_pairs P = pile_pairs_query(d, tid, 0);
    const int32_t cap = P.cap, found = P.found;
    const int32_t* pos = P.pos; const uint32_t* cnt = P.cnt;
    uint32_t* med = NULL;
    if (found > 0 && g_depth_evidence) {
        /* three queries per pair: the duplicated bases [pl, pr) and DEPTH_EV_FLANK bases on either side (the device clips to the contig) */
        int32_t* beg = xmalloc(sizeof(int32_t) * 6 * (size_t)found); int32_t* end = beg + 3 * (size_t)found;
        med = xmalloc(sizeof(uint32_t) * 3 * (size_t)found);
        for (int32_t k = 0; k < found; k++) {
            const int32_t pr = pos[k], pl = pos[cap + k];
            beg[3 * k] = pl; end[3 * k] = pr;
            beg[3 * k + 1] = pl - DEPTH_EV_FLANK; end[3 * k + 1] = pl;
            beg[3 * k + 2] = pr; end[3 * k + 2] = (int32_t)((int64_t)pr + DEPTH_EV_FLANK > INT32_MAX ? INT32_MAX : pr + DEPTH_EV_FLANK);
        }
        pthread_mutex_lock(&g_query_mu);
        const int qrc = d->pipe_mode ? im_depth_median_tid(d->gpu, tid, 3 * found, beg, end, med) : im_depth_median(d->gpu, 3 * found, beg, end, med);
        pthread_mutex_unlock(&g_query_mu);
        if (qrc != IM_OK) fatalf("im_depth_median: %s", im_last_error(d->gpu));
        free(beg);
    }
    uint32_t* pe = NULL;
    if (found > 0 && PAIRLINK_ON) {
        /* one query per pair: everted pairs, the leftmost read at the start of the duplicated bases, its mate in front of their end */
        uint8_t* kind = xmalloc((size_t)found); int32_t* win = xmalloc(sizeof(int32_t) * 4 * (size_t)found);
        for (int32_t k = 0; k < found; k++) {
            const int64_t pr = pos[k], pl = pos[cap + k];
            kind[k] = LINK_EVERTED;
            win[k] = link_clamp(pl - CLIPTAIL_MAX_SHIFT); win[found + k] = link_clamp(pl + LINK_EV_WINDOW);
            win[2 * found + k] = link_clamp(pr - LINK_EV_WINDOW); win[3 * found + k] = link_clamp(pr + CLIPTAIL_MAX_SHIFT);
        }
        pe = pair_links_query(d, tid, found, kind, win);
        free(kind); free(win);
    }
    /* -S: from (pl, the left clips) to (pr, the right clips), and back */
    uint32_t* sr = found > 0 && SPLITLINK_ON ? split_links_pairs(d, tid, found, pos + cap, pos, NULL, 1, 0) : NULL;
    const char* seq = d->sequences[tid];
    for (int32_t k = 0; k < found; k++) {
        const int32_t pr = pos[k], pl = pos[cap + k];
        if (pl == 0) continue;      /* nothing in front to anchor on */
        fprintf(f, "%s\t%d\t.\t%c\t<DUP:TANDEM>\t.\t.\tSVTYPE=DUP;END=%d;SVLEN=%d;HOMLEN=%d;CR=%u,%u;CN=%u,%u;CV=%u,%u", d->hdr->target_name[tid], pl,
                toupper((unsigned char)seq[pl - 1]), pr, pr - pl, pos[2 * cap + k], cnt[k], cnt[cap + k], cnt[4 * cap + k], cnt[5 * cap + k],
                cnt[2 * cap + k], cnt[3 * cap + k]);
        if (med) fprint_depth_values(f, med + 3 * k, ";DM=", ";DFC=");
        if (pe) fprint_pe(f, pe[k]);
        if (sr) fprint_sr(f, sr[k], sr[found + k]);
        fprintf(f, "\n");
    }
    free(med); free(pe); free(sr); free(P.pos); free(P.cnt);
}

static void inv_describe(FILE* f)
{
    fprintf(f, "##ALT=<ID=INV,Description=\"Inversion breakpoint: reads clipped on one side at POS and at END continue on the other strand at each other\">\n");
    fprintf(f, "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n");
    fprintf(f, "##INFO=<ID=END,Number=1,Type=Integer,Description=\"The second pile of clipped reads (POS: the first)\">\n");
    fprintf(f, "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"END - POS: bases inverted\">\n");
    fprintf(f, "##INFO=<ID=CT,Number=1,Type=String,Description=\"Junction: 3to3, both piles of reads that stop aligning with a clip (the left junction), or 5to5, both of reads that start aligning with one (the right junction)\">\n");
    fprintf(f, "##INFO=<ID=HOMLEN,Number=1,Type=Integer,Description=\"Bases by which the clipped reads continue behind the other breakpoint (micro-homology the aligner extended into, both piles together)\">\n");
    fprintf(f, "##INFO=<ID=CR,Number=2,Type=Integer,Description=\"Clipped reads at POS, clipped reads at END\">\n");
    fprintf(f, "##INFO=<ID=CN,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases were kept, either pile\">\n");
    fprintf(f, "##INFO=<ID=CV,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases are the reverse complement of the reference at the other pile\">\n");
    if (PAIRLINK_ON)
        fprintf(f, "##INFO=<ID=PE,Number=1,Type=Integer,Description=\"read pairs with both reads forward (CT=3to3: both start within %d bases in front of and %d behind POS "
                   "and END) or both reverse (CT=5to5: within %d in front of and %d behind), at least %d bases apart\">\n", LINK_EV_WINDOW, CLIPTAIL_MAX_SHIFT, CLIPTAIL_MAX_SHIFT, LINK_EV_WINDOW, LINK_EV_MIN_SEP);
    if (SPLITLINK_ON) sr_info(f);
    fprintf(f, "##inversion=\"a record per pair of positions POS < END, %d <= END - POS <= %d, at both of which at least %d reads of mapping quality >= -q stop aligning "
               "(CT=3to3) or at both of which such reads start aligning (CT=5to5) with a soft clip of at least %d bases, more than at any of the %d positions in front "
               "and no fewer than at any of the %d behind, when for one shift s in 0 .. %d at least %d of the reads at POS and at least %d of the reads at END "
               "continue with the complement of the reference running away from the other position, backwards from its base - 1 - s (3to3) or forwards from its "
               "base + s (5to5), in up to 32 clipped bases per read with at most 1 difference in 16 (HOMLEN: the s with the most such reads, the smallest among "
               "equals; CV: those reads); the two junctions of an inversion are two records; the file has no records once the clip-tail table has overflowed "
               "(stderr says so); POS 0 is skipped\"\n",
            INV_EV_MIN_LEN, INV_EV_MAX_LEN, INV_EV_MIN_READS, CLIP_EV_MIN_CLIP, INV_EV_REACH, INV_EV_REACH, CLIPTAIL_MAX_SHIFT, INV_EV_MIN_VERIFIED, INV_EV_MIN_VERIFIED);
    if (PAIRLINK_ON) pe_describe(f);
    if (SPLITLINK_ON) sr_describe(f);
}

/* -N: one contig's inverted piles into FILE.  No depth fields with -D: an inversion changes no depth. */
static void inv_contig(driver* d, int32_t tid, FILE* f)
{
    pile_pairs P = pile_pairs_query(d, tid, 1);
    const int32_t cap = P.cap;
    const int32_t* pos = P.pos; const uint32_t* cnt = P.cnt;
    uint32_t* pe = NULL;
    if (P.found > 0 && PAIRLINK_ON) {
        /* one query per junction: both reads forward in front of the two piles of a left junction, both reverse behind those of a right one */
        const int32_t n = P.found;
        uint8_t* kind = xmalloc((size_t)n); int32_t* win = xmalloc(sizeof(int32_t) * 4 * (size_t)n);
        for (int32_t k = 0; k < n; k++) {
            const int64_t x = pos[k], y = pos[cap + k];
            const int64_t lo = P.side[k] ? CLIPTAIL_MAX_SHIFT : LINK_EV_WINDOW, hi = P.side[k] ? LINK_EV_WINDOW : CLIPTAIL_MAX_SHIFT;
            kind[k] = P.side[k] ? LINK_REVERSE : LINK_FORWARD;
            win[k] = link_clamp(x - lo); win[n + k] = link_clamp(x + hi);
            win[2 * n + k] = link_clamp(y - lo); win[3 * n + k] = link_clamp(y + hi);
        }
        pe = pair_links_query(d, tid, n, kind, win);
        free(kind); free(win);
    }
    /* -S: from (x, the pair's side) to (y, the same side), and back */
    uint32_t* sr = P.found > 0 && SPLITLINK_ON ? split_links_pairs(d, tid, P.found, pos, pos + cap, P.side, 0, 0) : NULL;
    const char* seq = d->sequences[tid];
    for (int32_t k = 0; k < P.found; k++) {
        const int32_t x = pos[k], y = pos[cap + k];
        if (x == 0) continue;       /* nothing in front to anchor on */
        fprintf(f, "%s\t%d\t.\t%c\t<INV>\t.\t.\tSVTYPE=INV;END=%d;SVLEN=%d;CT=%s;HOMLEN=%d;CR=%u,%u;CN=%u,%u;CV=%u,%u", d->hdr->target_name[tid], x,
                toupper((unsigned char)seq[x - 1]), y, y - x, P.side[k] ? "5to5" : "3to3", pos[2 * cap + k], cnt[k], cnt[cap + k], cnt[4 * cap + k],
                cnt[5 * cap + k], cnt[2 * cap + k], cnt[3 * cap + k]);
        if (pe) fprint_pe(f, pe[k]);
        if (sr) fprint_sr(f, sr[k], sr[P.found + k]);
        fprintf(f, "\n");
    }
    free(pe); free(sr); free(P.pos); free(P.cnt); free(P.side);
}

/* -T: the FILE's ##ALT, ##INFO and description lines; the rule with its constants, as ##inversion= has it */
static void bnd_describe(FILE* f)
{
    fprintf(f, "##ALT=<ID=BND,Description=\"Breakend: reads clipped at POS continue on contig CHR2 at POS2\">\n");
    fprintf(f, "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">\n");
    fprintf(f, "##INFO=<ID=CHR2,Number=1,Type=String,Description=\"The contig of the second pile of clipped reads\">\n");
    fprintf(f, "##INFO=<ID=POS2,Number=1,Type=Integer,Description=\"The second pile of clipped reads (POS: the first, on the contig that comes first in the reference)\">\n");
    fprintf(f, "##INFO=<ID=CT,Number=1,Type=String,Description=\"Junction: 3 for a pile of reads that stop aligning with a clip, 5 for a pile of reads that start aligning with one; POS, then POS2\">\n");
    fprintf(f, "##INFO=<ID=HOMLEN,Number=1,Type=Integer,Description=\"Bases by which the clipped reads continue behind the other breakpoint (micro-homology the aligner extended into, both piles together)\">\n");
    fprintf(f, "##INFO=<ID=CR,Number=2,Type=Integer,Description=\"Clipped reads at POS, clipped reads at POS2\">\n");
    fprintf(f, "##INFO=<ID=CN,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases were kept, either pile\">\n");
    fprintf(f, "##INFO=<ID=CV,Number=2,Type=Integer,Description=\"Of those, the reads whose clipped bases are the other contig's at the other pile\">\n");
    fprintf(f, "##INFO=<ID=PE,Number=2,Type=Integer,Description=\"Read pairs that led from POS to POS2, read pairs that led from POS2 to POS: one read near the pile, its mate within two neighbouring cells of %d bases of the other contig; 0 where that pile's pairs point elsewhere or nowhere\">\n", BND_EV_CELL_BASES);
    if (SPLITLINK_ON) sr_info(f);
    fprintf(f, "##interContig=\"a record per pair of positions POS and POS2 on two contigs at each of which at least %d reads of mapping quality >= -q stop aligning (3) "
               "or start aligning (5) with a soft clip of at least %d bases, more than at any of the %d positions in front and no fewer than at any of the %d behind, "
               "when at least %d read pairs lead from one to the other and for one shift s in 0 .. %d at least %d of the reads at POS and at least %d of the reads at "
               "POS2 continue with the other contig at the other position, forwards from its base + s when that pile is of 5 reads and backwards from its base - 1 - s "
               "when it is of 3 reads, complemented when both piles are of one kind, in up to 32 clipped bases per read with at most 1 difference in 16 (HOMLEN: the s "
               "with the most such reads, the smallest among equals; CV: those reads); read pairs: paired, both reads mapped, neither secondary, supplementary, "
               "duplicate nor failing quality control, the mate on another contig, the read of mapping quality >= -q and on the strand of its pile (forward at 3, "
               "reverse at 5), starting within %d bases from the pile towards where its reads lie and %d the other way; the mates of one strand vote for the contig and "
               "the two neighbouring cells of %d bases most of them start in (at most %d cells: a pile whose mates scatter further has no partner), and the piles "
               "of that contig within %d and %d bases of those mates are tried; no genotype; the two junctions of a reciprocal translocation are two records; the "
               "mate's mapping quality is unknown; the file has no records once the clip-tail or the mate-link table has overflowed (stderr says so); POS 0 and "
               "POS2 0 are skipped\"\n",
            DUP_EV_MIN_READS, CLIP_EV_MIN_CLIP, DUP_EV_REACH, DUP_EV_REACH, BND_EV_MIN_LINKS, CLIPTAIL_MAX_SHIFT, BND_EV_MIN_VERIFIED, BND_EV_MIN_VERIFIED,
            LINK_EV_WINDOW, CLIPTAIL_MAX_SHIFT, BND_EV_CELL_BASES, IM_MATELINK_CELLS, LINK_EV_WINDOW, CLIPTAIL_MAX_SHIFT);
    if (SPLITLINK_ON) sr_describe(f);
}

/* the peaks of one clip array of one contig, ascending */
typedef struct bnd_peaks { int32_t n; int32_t* pos; uint32_t* cnt; int32_t* mtid; uint32_t* np; int32_t* lo; int32_t* hi; } bnd_peaks;
/* a junction: end 1 is the lower (tid, position); n1, n2: the pairs that led to it from either end */
typedef struct bnd_junction { int32_t tid1, p1, tid2, p2; uint8_t s1, s2; uint32_t c1, c2, n1, n2; } bnd_junction;

static int bnd_cmp(const void* a, const void* b)
{
    const bnd_junction* x = a; const bnd_junction* y = b;
    if (x->tid1 != y->tid1) return x->tid1 < y->tid1 ? -1 : 1;
    if (x->p1 != y->p1) return x->p1 < y->p1 ? -1 : 1;
    if (x->tid2 != y->tid2) return x->tid2 < y->tid2 ? -1 : 1;
    if (x->p2 != y->p2) return x->p2 < y->p2 ? -1 : 1;
    if (x->s1 != y->s1) return x->s1 < y->s1 ? -1 : 1;
    if (x->s2 != y->s2) return x->s2 < y->s2 ? -1 : 1;
    return 0;
}

/* -T: every contig's peaks, their partner queries, the candidates those name, the junction verify, FILE.  Once per run, on either
 * path, when every scatter has completed: the clip arrays are genome-wide and the tables are keyed by contig.  The lists are small
 * and stay on the host; every device call is under g_query_mu. */
static void bnd_search(driver* d)
{
    FILE* f = fopen(g_bnd_file, "w");
    if (!f) fatalf("cannot write %s", g_bnd_file);
    fprintf(f, "##fileformat=VCFv4.1\n");
    bnd_describe(f);
    fprintf(f, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n");
    gpu_wait(d);
    uint64_t stored = 0, dropped_tail = 0, dropped_mate = 0;
    pthread_mutex_lock(&g_query_mu);
    if (im_cliptail_stats(d->gpu, &stored, &dropped_tail) != IM_OK) fatalf("im_cliptail_stats: %s", im_last_error(d->gpu));
    if (im_matelink_stats(d->gpu, &stored, &dropped_mate) != IM_OK) fatalf("im_matelink_stats: %s", im_last_error(d->gpu));
    pthread_mutex_unlock(&g_query_mu);
    const int32_t nt = d->hdr->n_targets;
    if (dropped_tail == 0 && dropped_mate == 0 && nt > 1) {
        /* 1, 2: the peaks of both arrays, and per peak the partner of its reads' mates on either strand (m = 0, then m = 1) */
        bnd_peaks* P = xcalloc(2 * (size_t)nt, sizeof(bnd_peaks));
        for (int32_t tid = 0; tid < nt; tid++) {
            for (int side = 0; side < 2; side++) {
                bnd_peaks* p = &P[2 * tid + side];
                int32_t cap = 4096, found = 0;
                pthread_mutex_lock(&g_query_mu);
                for (;; cap = found) {
                    p->pos = xrealloc(p->pos, sizeof(int32_t) * (size_t)cap); p->cnt = xrealloc(p->cnt, sizeof(uint32_t) * (size_t)cap);
                    if (im_clip_peaks_tid(d->gpu, tid, side, DUP_EV_MIN_READS, DUP_EV_REACH, cap, p->pos, p->cnt, &found) != IM_OK)
                        fatalf("im_clip_peaks_tid: %s", im_last_error(d->gpu));
                    if (found <= cap) break;
                }
                p->n = found > 0 ? found : 0;
                if (p->n > 0) {
                    const size_t n = (size_t)p->n;
                    uint8_t* kind = xmalloc(2 * n); int32_t* win = xmalloc(sizeof(int32_t) * 4 * n); uint32_t* nl = xmalloc(sizeof(uint32_t) * 2 * n);
                    p->mtid = xmalloc(sizeof(int32_t) * 2 * n); p->np = xmalloc(sizeof(uint32_t) * 2 * n);
                    p->lo = xmalloc(sizeof(int32_t) * 2 * n); p->hi = xmalloc(sizeof(int32_t) * 2 * n);
                    for (size_t k = 0; k < 2 * n; k++) {
                        const int64_t at = p->pos[k % n];
                        const int m = k >= n;
                        kind[k] = (uint8_t)(side | m << 1);
                        win[k] = link_clamp(at - (side ? CLIPTAIL_MAX_SHIFT : LINK_EV_WINDOW));
                        win[2 * n + k] = link_clamp(at + (side ? LINK_EV_WINDOW : CLIPTAIL_MAX_SHIFT));
                    }
                    if (im_matelink_partner(d->gpu, tid, (int32_t)(2 * n), kind, win, win + 2 * n, nl, p->mtid, p->np, p->lo, p->hi) != IM_OK)
                        fatalf("im_matelink_partner: %s", im_last_error(d->gpu));
                    free(kind); free(win); free(nl);
                }
                pthread_mutex_unlock(&g_query_mu);
            }
        }
        /* 3: the candidates -- the peaks of array side2 = m on the partner contig inside the window around its mates; each junction once,
         * with the pairs that led to it from either end */
        bnd_junction* J = NULL; size_t nj = 0, capj = 0;
        for (int32_t tid = 0; tid < nt; tid++) {
            for (int side = 0; side < 2; side++) {
                const bnd_peaks* p = &P[2 * tid + side];
                for (int32_t k = 0; k < 2 * p->n; k++) {
                    const int m = k >= p->n;
                    const int32_t at = k % p->n, mt = p->mtid[k];
                    if (mt < 0 || mt >= nt || p->np[k] < BND_EV_MIN_LINKS) continue;
                    const bnd_peaks* o = &P[2 * mt + m];
                    const int64_t w0 = (int64_t)p->lo[k] - (m ? LINK_EV_WINDOW : CLIPTAIL_MAX_SHIFT), w1 = (int64_t)p->hi[k] + (m ? CLIPTAIL_MAX_SHIFT : LINK_EV_WINDOW);
                    for (int32_t j = 0; j < o->n; j++) {
                        if (o->pos[j] < w0 || o->pos[j] > w1) continue;
                        bnd_junction x;
                        const int first = tid < mt;         /* mt != tid: a mate link names another contig */
                        x.tid1 = first ? tid : mt; x.p1 = first ? p->pos[at] : o->pos[j]; x.s1 = (uint8_t)(first ? side : m); x.c1 = first ? p->cnt[at] : o->cnt[j];
                        x.tid2 = first ? mt : tid; x.p2 = first ? o->pos[j] : p->pos[at]; x.s2 = (uint8_t)(first ? m : side); x.c2 = first ? o->cnt[j] : p->cnt[at];
                        x.n1 = first ? p->np[k] : 0; x.n2 = first ? 0 : p->np[k];
                        size_t e = 0;
                        while (e < nj && bnd_cmp(&J[e], &x) != 0) e++;
                        if (e < nj) { J[e].n1 += x.n1; J[e].n2 += x.n2; continue; }     /* found from the other end: one query per end leads here */
                        if (nj == capj) { capj = capj ? 2 * capj : 64; J = xrealloc(J, sizeof(bnd_junction) * capj); }
                        J[nj++] = x;
                    }
                }
            }
        }
        /* 4 .. 6: verify, keep, sort, print */
        if (nj > 0) {
            qsort(J, nj, sizeof(bnd_junction), bnd_cmp);
            int32_t* q = xmalloc(sizeof(int32_t) * 5 * nj); uint8_t* qs = xmalloc(2 * nj); uint32_t* a = xmalloc(sizeof(uint32_t) * 4 * nj);
            for (size_t k = 0; k < nj; k++) {
                q[k] = J[k].tid1; q[nj + k] = J[k].p1; q[2 * nj + k] = J[k].tid2; q[3 * nj + k] = J[k].p2; qs[k] = J[k].s1; qs[nj + k] = J[k].s2;
            }
            pthread_mutex_lock(&g_query_mu);
            const int rc = im_cliptail_junction(d->gpu, (int32_t)nj, q, q + nj, qs, q + 2 * nj, q + 3 * nj, qs + nj, CLIPTAIL_MAX_SHIFT, a, a + nj, q + 4 * nj,
                                                a + 2 * nj, a + 3 * nj);
            pthread_mutex_unlock(&g_query_mu);
            if (rc != IM_OK) fatalf("im_cliptail_junction: %s", im_last_error(d->gpu));
            /* -S: from end 1 to end 2 of every junction, and back: one call for the FILE */
            uint32_t* sr = SPLITLINK_ON ? split_links_query(d, (int32_t)nj, q, q + nj, qs, q + 2 * nj, q + 3 * nj, qs + nj) : NULL;
            static const char* const ct[2][2] = {{"3to3", "3to5"}, {"5to3", "5to5"}};
            for (size_t k = 0; k < nj; k++) {
                const bnd_junction* x = &J[k];
                const uint32_t v1 = a[k], v2 = a[nj + k];
                if (v1 == CLIPTAIL_NONE || v1 < BND_EV_MIN_VERIFIED || v2 < BND_EV_MIN_VERIFIED) continue;
                if (x->p1 == 0 || x->p2 == 0) continue;    /* nothing in front to anchor on */
                const char* c1 = d->hdr->target_name[x->tid1]; const char* c2 = d->hdr->target_name[x->tid2];
                const int ref = toupper((unsigned char)d->sequences[x->tid1][x->p1 - 1]);
                fprintf(f, "%s\t%d\t.\t%c\t", c1, x->p1, ref);
                if (!x->s1 && x->s2) fprintf(f, "%c[%s:%d[", ref, c2, x->p2);
                else if (x->s1 && !x->s2) fprintf(f, "]%s:%d]%c", c2, x->p2, ref);
                else if (!x->s1) fprintf(f, "%c]%s:%d]", ref, c2, x->p2);
                else fprintf(f, "[%s:%d[%c", c2, x->p2, ref);
                fprintf(f, "\t.\t.\tSVTYPE=BND;CHR2=%s;POS2=%d;CT=%s;HOMLEN=%d;CR=%u,%u;CN=%u,%u;CV=%u,%u;PE=%u,%u", c2, x->p2, ct[x->s1][x->s2], q[4 * nj + k],
                        x->c1, x->c2, a[2 * nj + k], a[3 * nj + k], v1, v2, x->n1, x->n2);
                if (sr) fprint_sr(f, sr[k], sr[nj + k]);
                fprintf(f, "\n");
            }
            free(q); free(qs); free(a); free(sr);
        }
        free(J);
        for (int32_t k = 0; k < 2 * nt; k++) { free(P[k].pos); free(P[k].cnt); free(P[k].mtid); free(P[k].np); free(P[k].lo); free(P[k].hi); }
        free(P);
    }
    if (fclose(f) != 0) fatalf("cannot write %s", g_bnd_file);
    phase_time("inter-contig breakpoint evidence (device)");
}

/* -J's header: a line per INFO key, and the whole rule with its constants */
static void junc_describe(FILE* f)
{
    fprintf(f, "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant: BND, one junction between two ends\">\n"
               "##INFO=<ID=CHR2,Number=1,Type=String,Description=\"Contig of the second end\">\n"
               "##INFO=<ID=POS2,Number=1,Type=Integer,Description=\"Position of the second end\">\n"
               "##INFO=<ID=CT,Number=1,Type=String,Description=\"Which side of either end the junction joins: 3 = the reads there are clipped on their right, 5 = on their left\">\n"
               "##INFO=<ID=JT,Number=1,Type=String,Description=\"What a junction of this CT on these contigs is read as: TRA on two contigs; on one, DEL for 3to5, DUP for 5to3, "
               "INV for 3to3 and 5to5\">\n"
               "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"POS2 - POS, on one contig only\">\n"
               "##INFO=<ID=SE,Number=1,Type=Integer,Description=\"Split reads that name exactly these two ends, from either\">\n");
    fprintf(f, "##INFO=<ID=SR,Number=2,Type=Integer,Description=\"Split reads whose primary part ends within %d bases of the first end and whose SA tag "
               "places the clipped part within %d bases of the second, and the same from the second to the first\">\n", SPLIT_EV_WINDOW, SPLIT_EV_WINDOW);
    if (JUNCOVL_ON)
        fprintf(f, "##INFO=<ID=HOMLEN,Number=1,Type=Integer,Description=\"Micro-homology at the junction: the read bases that both parts of a split read align, "
                   "the lower median over the reads of SR that state it; 0 when that median is an insertion\">\n"
                   "##INFO=<ID=INSLEN,Number=1,Type=Integer,Description=\"Inserted bases at the junction: the read bases between the two parts of a split read that "
                   "neither aligns, from the same median; 0 when it is a homology\">\n"
                   "##INFO=<ID=OA,Number=2,Type=Integer,Description=\"Overlap agreement: the reads of SR whose own overlap equals that median, and the reads of SR "
                   "that state one\">\n");
    if (JUNCPAIR_ON)
        fprintf(f, "##INFO=<ID=PE,Number=.,Type=Integer,Description=\"Read pairs across the junction: on one contig the pairs of the junction's orientation with "
                   "one read at either end; on two contigs the pairs counted from the first end and from the second\">\n");
    if (JUNCGT_ON)
        fprintf(f, "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype of the junction, the most likely of 0/0, 0/1, 1/1 given AD\">\n"
                   "##FORMAT=<ID=AD,Number=2,Type=Integer,Description=\"Read support of the reference and the junction allele: RS, the smaller number of RB (for JT=DUP "
                   "less the second number here, not below 0), and the sum of the two numbers of SR\">\n"
                   "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: phred-scaled distance to the second most likely genotype, at most 99\">\n"
                   "##FORMAT=<ID=RB,Number=2,Type=Integer,Description=\"Alignments that match the reference for the -n distance on both sides of the boundary behind "
                   "base POS, and of the one behind base POS2\">\n");
    fprintf(f, "##splitJunctions=\"junctions from split reads alone: a split read is a primary record at or above -q whose soft clip at either end has %d bases "
               "or more and whose SA tag holds exactly one entry, itself at or above -q, that continues the read; it names two ends (contig, position, side); "
               "an end pair on two contigs, or on one contig %d bases or more apart, is a candidate, its read count SE the reads that name exactly its two ends from "
               "either; a candidate is kept when no candidate of the same contigs and sides within %d bases at both ends has a larger SE, or the same SE and a "
               "smaller POS, then a smaller POS2 (a candidate that loses stays lost when its winner loses to a third); SR counts every split read between the "
               "windows of %d bases around the two ends, from the first and from the second; a kept candidate needs SR of %d in sum; no clip pile and no "
               "comparison with the reference is needed, so a junction with inserted bases, with micro-homology above %d bases or with reads clipped at "
               "scattered positions is reported; nothing is merged with or filtered against the records of -U, -N and -T; %s; a tag with several "
               "entries stores nothing; the file has no records once the split-link table has overflowed (stderr says so); POS 0 and POS2 0 are skipped\"\n",
            CLIP_EV_MIN_CLIP, JUNC_EV_MIN_SPAN, SPLIT_EV_WINDOW, SPLIT_EV_WINDOW, JUNC_EV_MIN_LINKS, CLIPTAIL_MAX_SHIFT,
            JUNCGT_ON ? "the genotype is that of ##junctionGenotype" : "no genotype");
    if (JUNCGT_ON)
        fprintf(f, "##junctionGenotype=\"every junction against the reads that run through its two ends on the reference allele: ALT is the sum of the two numbers of SR "
                   "(a split read stores one link, at its primary record, so the two are disjoint sets of reads); RB=RS1,RS2 are -G's count of alignments at or above -q "
                   "that match the reference for the -n distance on both sides, the smallest within %d bases of the boundary behind base POS and of the one behind "
                   "base POS2, which is where a clip on either side puts the junction (a split read's own alignment ends there and is in neither); RS is the "
                   "smaller of RS1 and RS2, except for JT=DUP, where RS is that less ALT and not below 0: a tandem duplication keeps both outer boundaries of the "
                   "duplicated segment intact on the duplicated allele, so every copy of that allele adds reference-looking reads at POS and at POS2 at the rate at which "
                   "it adds split reads, and a homozygous duplication would show RS about ALT and never be called 1/1; GT and GQ are -G's, the same integers from AD=RS,ALT; "
                   "a reference read must hold -n bases on either side while a split read needs a clip of %d bases and a placed remainder, so the two alleles are not "
                   "equally detectable and nothing corrects for it; RS is exact for one position while micro-homology lets an aligner place the split anywhere inside it; "
                   "a read with an indel near an end may count on neither side; the two junctions of an inversion or of a reciprocal translocation are genotyped "
                   "independently; the records of -U, -N and -T have no genotype\"\n", JUNC_GT_SLACK, CLIP_EV_MIN_CLIP);
    if (JUNCOVL_ON)
        fprintf(f, "##junctionOverlap=\"every split read states its own overlap d in its two CIGARs: with L1, T1 the clipped bases (S and H) in front of and behind "
                   "the primary alignment, L2, T2 those of the SA entry (exchanged when the entry is on the other strand), Q1 = L1 + T1 + the primary's M, I, = and X "
                   "bases and Q2 the entry's M, I, S, H, = and X bases, d = Q1 - T1 - L2 when the entry aligns the bases behind the primary's and d = Q1 - T2 - L1 "
                   "when it aligns those in front; d above 0 is that many read bases aligned by both parts (micro-homology), d below 0 that many aligned by "
                   "neither (inserted bases), 0 a clean junction; a read with Q1 other than Q2 or with d outside -%d .. %d states none; over the reads of "
                   "SR, from either end, within %d bases at both ends, that state one, OA=agree,known gives their number and how many equal their lower "
                   "median (the element of index (known - 1) / 2 in ascending order), HOMLEN is that median when above 0 and INSLEN its negative when below, "
                   "each 0 otherwise; HOMLEN=.;INSLEN=.;OA=0,0 when no read states one; no inserted sequence is printed (that needs read bases), there is "
                   "no CIPOS, d is what the aligner says and is not compared with the reference, so a junction above %d bases of homology is described as well; "
                   "the records of -U, -N and -T are not touched\"\n", 32767, 32767, SPLIT_EV_WINDOW, CLIPTAIL_MAX_SHIFT);
    if (JUNCPAIR_ON)
        fprintf(f, "##junctionPairs=\"every junction against the read pairs on either side of it, which come from other molecules than the split reads of SE and SR: "
                   "a record counts when it is paired, mapped with a mapped mate, primary, no duplicate and no failure, at or above -q (its mate's quality is not "
                   "known); an end with CT 3 is supported by forward reads that start from %d bases in front of it to %d behind, an end with CT 5 by reverse reads "
                   "that start from %d in front of it to %d behind; on one contig PE=n counts the pairs whose leftmost read supports the end with the smaller position "
                   "(POS on a tie) and whose mate supports the other, their starts at least %d bases apart: JT=DUP reverse then forward, JT=INV both forward (3to3) "
                   "or both reverse (5to5), and JT=DEL forward then reverse, the normal orientation, only when the aligner has NOT flagged the pair a proper pair "
                   "(flag 0x2 clear) -- its verdict stands in for an insert-size test, so a deletion shorter than the spread of the library's insert size leaves "
                   "proper pairs and PE=0 is expected there; on two contigs PE=n1,n2 counts the pairs with a read that supports the first end and its mate "
                   "supporting the second, at the record of the first end's read and at that of the second end's; PE=. or PE=.,. once that table has "
                   "overflowed (stderr says so); a duplication or an inversion shorter than a read leaves no such pair; nothing is filtered by PE, and the "
                   "ALT of ##junctionGenotype stays the split reads alone; the records of -U, -N and -T are not touched\"\n",
                LINK_EV_WINDOW, CLIPTAIL_MAX_SHIFT, CLIPTAIL_MAX_SHIFT, LINK_EV_WINDOW, LINK_EV_MIN_SEP);
}

/* -J: the device's search over the table of split links, FILE.  Once per run, on either path, when every scatter has completed.  One
 * call under g_query_mu, asked again with the cap it names while that exceeds the one it was given. */
static void junc_search(driver* d)
{
    FILE* f = fopen(g_junc_file, "w");
    if (!f) fatalf("cannot write %s", g_junc_file);
    fprintf(f, "##fileformat=VCFv4.1\n");
    junc_describe(f);
    if (JUNCGT_ON) fprintf(f, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t%s\n", g_sample_name);
    else fprintf(f, "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n");
    gpu_wait(d);
    int32_t cap = 4096, found = 0;
    int32_t* q = NULL; uint8_t* qs = NULL; uint32_t* a = NULL; uint32_t* rb = NULL;
    pthread_mutex_lock(&g_query_mu);
    for (;; cap = found) {
        const size_t n = (size_t)cap;
        q = xrealloc(q, sizeof(int32_t) * 4 * n); qs = xrealloc(qs, 2 * n); a = xrealloc(a, sizeof(uint32_t) * 3 * n);
        if (im_splitlink_junctions(d->gpu, SPLIT_EV_WINDOW, JUNC_EV_MIN_LINKS, JUNC_EV_MIN_SPAN, cap, q, q + n, qs, q + 2 * n, q + 3 * n, qs + n, a, a + n, a + 2 * n,
                                   &found) != IM_OK)
            fatalf("im_splitlink_junctions: %s", im_last_error(d->gpu));
        if (found <= cap) break;
    }
    /* -K: the reference side of every end, the first ends then the second ones, in one call behind the search.  Every contig's run of
     * span[] holds counts by now: either path scans a contig when its last record has been scattered, and this runs behind both */
    if (JUNCGT_ON && found > 0) {
        const size_t n = (size_t)cap, m = (size_t)found;
        int32_t* et = xmalloc(sizeof(int32_t) * 4 * m);
        rb = xmalloc(sizeof(uint32_t) * 2 * m);
        memcpy(et, q, sizeof(int32_t) * m); memcpy(et + m, q + 2 * n, sizeof(int32_t) * m);                     /* tid1, tid2 */
        memcpy(et + 2 * m, q + n, sizeof(int32_t) * m); memcpy(et + 3 * m, q + 3 * n, sizeof(int32_t) * m);     /* pos1, pos2 */
        if (im_span_query_ends(d->gpu, (int32_t)(2 * m), et, et + 2 * m, JUNC_GT_SLACK, rb) != IM_OK)
            fatalf("im_span_query_ends: %s", im_last_error(d->gpu));
        free(et);
    }
    /* -H: the overlaps of every junction's links, in one call behind the search: known, median, agree */
    uint32_t* ov = NULL;
    if (JUNCOVL_ON && found > 0) {
        const size_t n = (size_t)cap, m = (size_t)found;
        ov = xmalloc(sizeof(uint32_t) * 3 * m);
        if (im_splitlink_overlap(d->gpu, found, q, q + n, qs, q + 2 * n, q + 3 * n, qs + n, SPLIT_EV_WINDOW, ov, (int32_t*)(ov + m), ov + 2 * m) != IM_OK)
            fatalf("im_splitlink_overlap: %s", im_last_error(d->gpu));
    }
    /* -E: the read pairs on either side of every junction, out of both pair tables in one call behind that: pe1, pe2 */
    uint32_t* pe = NULL;
    if (JUNCPAIR_ON && found > 0) {
        const size_t n = (size_t)cap, m = (size_t)found;
        pe = xmalloc(sizeof(uint32_t) * 2 * m);
        if (im_junction_pairs(d->gpu, found, q, q + n, qs, q + 2 * n, q + 3 * n, qs + n, LINK_EV_WINDOW, CLIPTAIL_MAX_SHIFT, LINK_EV_MIN_SEP, pe, pe + m) != IM_OK)
            fatalf("im_junction_pairs: %s", im_last_error(d->gpu));
    }
    pthread_mutex_unlock(&g_query_mu);
    static const char* const ct[2][2] = {{"3to3", "3to5"}, {"5to3", "5to5"}};
    const size_t n = (size_t)cap;
    for (int32_t k = 0; k < found; k++) {                       /* found = -1: the table has overflowed, the header alone */
        const int32_t tid1 = q[k], p1 = q[n + k], tid2 = q[2 * n + k], p2 = q[3 * n + k];
        const int s1 = qs[k], s2 = qs[n + k];
        if (p1 == 0 || p2 == 0) continue;                       /* nothing in front to anchor on */
        const char* c1 = d->hdr->target_name[tid1]; const char* c2 = d->hdr->target_name[tid2];
        const int ref = toupper((unsigned char)d->sequences[tid1][p1 - 1]);
        fprintf(f, "%s\t%d\t.\t%c\t", c1, p1, ref);
        if (!s1 && s2) fprintf(f, "%c[%s:%d[", ref, c2, p2);
        else if (s1 && !s2) fprintf(f, "]%s:%d]%c", c2, p2, ref);
        else if (!s1) fprintf(f, "%c]%s:%d]", ref, c2, p2);
        else fprintf(f, "[%s:%d[%c", c2, p2, ref);
        const char* jt = tid1 != tid2 ? "TRA" : s1 == s2 ? "INV" : s1 ? "DUP" : "DEL";
        fprintf(f, "\t.\t.\tSVTYPE=BND;CHR2=%s;POS2=%d;CT=%s;JT=%s", c2, p2, ct[s1][s2], jt);
        if (tid1 == tid2) fprintf(f, ";SVLEN=%d", p2 - p1);
        fprintf(f, ";SE=%u;SR=%u,%u", a[k], a[n + k], a[2 * n + k]);
        if (JUNCOVL_ON) {
            /* "Junction overlap": the lower median of the reads that state one; above 0 a homology, below 0 an insertion */
            const uint32_t known = ov[k], agree = ov[2 * (size_t)found + k];
            const int32_t med = (int32_t)ov[(size_t)found + k];
            if (known == 0) fprintf(f, ";HOMLEN=.;INSLEN=.;OA=0,0");
            else fprintf(f, ";HOMLEN=%d;INSLEN=%d;OA=%u,%u", med > 0 ? med : 0, med < 0 ? -med : 0, agree, known);
        }
        if (JUNCPAIR_ON) {
            /* "Junction pairs": one number on one contig, one from either end on two; the table's overflow blanks both */
            const uint32_t n1 = pe[k], n2 = pe[(size_t)found + k];
            if (tid1 == tid2) { if (n1 == JUNCPAIR_NONE) fprintf(f, ";PE=."); else fprintf(f, ";PE=%u", n1); }
            else if (n1 == JUNCPAIR_NONE) fprintf(f, ";PE=.,.");
            else fprintf(f, ";PE=%u,%u", n1, n2);
        }
        if (JUNCGT_ON) {
            /* "Junction genotypes": the smaller of the two ends; a tandem duplication's own reads run through both, so they come off */
            const int64_t rs1 = rb[k], rs2 = rb[found + k], alt = (int64_t)a[n + k] + a[2 * n + k];
            int64_t rs = rs1 < rs2 ? rs1 : rs2;
            if (tid1 == tid2 && s1 && !s2) rs = rs > alt ? rs - alt : 0;
            int best, gq;
            genotype_of(rs, alt, &best, &gq);
            fprintf(f, "\tGT:AD:GQ:RB\t%s:%lld,%lld:%d:%lld,%lld", best == 0 ? "0/0" : best == 1 ? "0/1" : "1/1", (long long)rs, (long long)alt, gq,
                    (long long)rs1, (long long)rs2);
        }
        fprintf(f, "\n");
    }
    free(q); free(qs); free(a); free(rb); free(ov); free(pe);
    if (fclose(f) != 0) fatalf("cannot write %s", g_junc_file);
    phase_time("split-link junctions (device)");
}

static void run_contig(driver* d, int32_t tid, int32_t beg, int32_t end, bgzf_reader* r)
{
    d->n_items = 0; d->n_flushes = 0;
    cb_reset(&d->cb);
    bam_region_iter it;
    bam_record b; memset(&b, 0, sizeof b);
    if (bam_region_begin(&it, r, d->idx, tid, beg, end) != 0) fatalf("cannot seek in %s", d->bam_name);
    d->segs.n = 0;
    host_chunk_init(d);
    const int whole = (beg <= 0 && end >= d->hdr->target_len[tid]);
    volatile int died = 0;              /* a record the reference dies on ended the pass: the flushes in front of it are still to print */
    t_is_main_thread_of_passA = 1;
    if (setjmp(g_passA_jmp)) died = 1;
    else g_passA_armed = 1;
    while (!died && host_chunk_next(d, &it, &b)) {
        if (whole && b.tid >= 0 && !(b.flag & (0x4 | 0x100 | 0x200 | 0x400))) {
            /* what samtools' pileup would count for DP= (bam_pileup.c:171-172,238-265) */
            const uint8_t* cig = BAMR_CIGAR(&b);
            int32_t x = b.pos;
            for (int kk = 0; kk < b.n_cigar; kk++) {
                const int op = CIG_OP(bamr_cigar_at(cig, kk)), len = CIG_LEN(bamr_cigar_at(cig, kk));
                if (op == OP_M || op == OP_EQ || op == OP_X) {
                    ivl_push(&d->segs, x, len);
                    x += len;
                } else if (op == OP_D || op == OP_N) x += len;
            }
            if (x - b.pos > g_longest_span) note_span(x - b.pos);       /* how far in front of a DP= window the deepest position is looked for */
        }
        dispatch_record(d, &b);
    }
    g_passA_armed = 0;
    /* the last records go out now, the record the reference died on among them (the chunk is the driver's: it outlives the jump) */
    host_chunk_submit(d);
    phase_time("pass A (BAM decode + dispatch)");
    d->depth_tid = -1;
    if (whole) {
        gpu_wait(d);
        if (im_depth_build(d->gpu, d->seqlen[tid], (int32_t)d->segs.n, d->segs.start, d->segs.len) != IM_OK)
            fatalf("im_depth_build: %s", im_last_error(d->gpu));
        d->depth_tid = tid;
    }
    phase_time("depth array (device)");
    /* -G, -A, -P: the contig's stretch of the scattered difference arrays becomes counts; the clip arrays and the tables need nothing */
    if (SPAN_ON) GPU2(d, im_span_scan(d->gpu, tid, im_ctx_stream(d->gpu)));
    if (PAIR_ON) GPU2(d, im_pairspan_scan(d->gpu, tid, im_ctx_stream(d->gpu)));
    if (SPAN_ON || PAIR_ON) GPU2(d, im_stream_sync(d->gpu, im_ctx_stream(d->gpu)));
    phase_time("evidence arrays (device)");

    im_read_result* res = NULL;
    if (d->cb.n > 0) {
        im_params P = { O.klength, O.numgaps, O.maxdelsize, O.ethreshold };
        im_read_batch batch = { d->cb.n, d->cb.bases, d->cb.base_off, d->cb.tid, d->cb.anchor, d->cb.range_max };
        res = xmalloc(sizeof(im_read_result) * (size_t)d->cb.n);
        gpu_wait(d);
        const int rc = im_realign_batch(d->gpu, &P, &batch, res);
        if (rc != IM_OK) fatalf("im_realign_batch: %s", im_last_error(d->gpu));
    }
    phase_time("realign batch (device, incl. copies)");
    int f = 0;
    for (int64_t i = 0; i <= d->n_items; i++) {
        while (f < d->n_flushes && d->flushes[f].n_items == i) {
            flush_variants(d, d->flushes[f].tid, d->flushes[f].marker);
            f++;
        }
        if (i == d->n_items) break;
        const item_t* itm = &d->items[i];
        if (itm->kind == ITEM_CAND) { resolve_candidate(d, itm, &res[itm->cand], tid); free(itm->bwa); }
        else pending_push(d, itm->pe);
    }
    free(res);
    if (died) {
        /* what the reference had printed when it met the record is out; its message and status follow */
        out_flush_on_exit();
        fflush(stdout);
        if (g_passA_msg[0] == 1) fprintf(stderr, "%s\n", g_passA_msg + 1);     /* an assertion's own form */
        else fprintf(stderr, "indelminer: %s\n", g_passA_msg);
        exit(EXIT_FAILURE);
    }
    flush_variants(d, tid, INT_MAX);        /* end of contig (src/indelminer.c:806-823) */
    phase_time("pass B (cluster, merge, print)");
    if (g_vcfname != NULL) {
        print_known_rest(d, &g_known);       /* what print_knownvariants left over (src/indelminer.c:839-847) */
    }
}

/* multi-GPU state (the section further down): declared here because the replay writes one part per contig */
#define MG_MAX_RG    64
#define MG_RG_WORDS  18         /* name[48] + min + max + first_tid + first position + seen on a proper pair + first record */

typedef struct {
    int rank, world, local_rank;
    im_comm* comm;
    char dir[400];
    int32_t* owner;             /* [n_targets] the rank that walks the contig (mg_plan) */
    int64_t* piece_prefix;      /* [pieces] counted reads of the run in front of each piece */
    int32_t* claim_walker;      /* [claims] the rank that walks the claim (reads the file, runs the triage) */
    int32_t* piece_walker;      /* [pieces] the same per piece */
    int32_t* claim_owner;       /* [claims] the rank that stages and replays it: the owner of its contig */
    int      split;             /* some claim is walked by a rank that does not own it (pieces of a contig over several GPUs) */
    int*     floor;             /* [n_targets] smallest start of a stale pair-table entry of an earlier contig */
    int      out_fd;            /* rank 0: the real stdout */
    uint8_t* skip;              /* [n_targets] annotate mode: contigs without known variants are not walked at all */
    int      abort_tid;         /* -1, or the first contig of this rank that holds a record the reference dies on */
    int      cross;             /* the exchanged pair-table logs show entries of one contig meeting records of another */
    int      abort_piece;       /* the first piece (plan index) whose walk some rank did not survive; the number of pieces: none */
} mgpu;

static mgpu* g_mg = NULL;
static int g_mg_self_ship = 0;          /* tests: claims this rank owns AND walks go through the exchange too */
static driver* g_mg_driver = NULL;
static void mg_finish(mgpu* m, driver* d);
static int g_mg_cur_tid = -1;          /* the first contig of the claim the main thread is working on */

static void mg_path(const mgpu* m, char* out, size_t cap, const char* what, int idx) { snprintf(out, cap, "%s/%s.%d", m->dir, what, idx); }
