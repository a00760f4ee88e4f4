/* host_main.c -- part of the indelminer host driver (one translation unit: imhost.c includes the parts in order, so that the
 * reference-shaped helpers can stay static).  Here: usage, option parsing, main. */

/* -------------------------------------------------------------------- main -- */

static void print_help(FILE* file)
{
    /* src/indelminer.c:883-923 */
    fprintf(file, "\n");
    fprintf(file, "Program: indelminer (Call/Tag indels from a clean BAM file)\n");
    fprintf(file, "Version: %2.2f\n\n", INDELMINER_VERSION);
    fprintf(file, "Usage:\n");
    fprintf(file, "\tindelminer [options] ref.fa [indels.vcf] sample=aln.bam\n");
    fprintf(file, "where the options are\n");
    fprintf(file, "\t-h   print help and return\n");
    fprintf(file, "\n");
    fprintf(file, "\t-i, read the configuration from this file\n");
    fprintf(file, " \t-c, only analyze this chromosomal region [ALL]\n");
    fprintf(file, " \t-t, do not call indels on 3' regions of the read\n");
    fprintf(file, " \t-q, do not call indels from reads with MQ < INT [10]\n");
    fprintf(file, " \t-n, disallow indel within INT bp towards the ends [10]\n");
    fprintf(file, " \t    We ignore the 3' soft-clipping, since that is where\n");
    fprintf(file, " \t    we expect the low quality region on the reads\n");
    fprintf(file, "\t-a, in case of overlapping indels, call all of them\n");
    fprintf(file, "\t    Default is to call the indels with most support\n");
    fprintf(file, "\t-e, minimum support for an indel [2]\n");
    fprintf(file, "\t-o, output format. vcf/detailed [vcf]\n");
    fprintf(file, "\t-s, maximum size of deletion reported using split reads [1 kbp]\n");
    fprintf(file, "\t-p, maximum size of deletion reported using PE reads [1 Mbp]\n");
    fprintf(file, "\n");
    fprintf(file, "\t-k, length of the kmers to be used in alignments[6]\n");
    fprintf(file, "\t-g, number of gaps allowed in the alignments[0]\n");
    fprintf(file, "\t-f, number of differences allowed in an alignment[6]\n");
    fprintf(file, "\t-b, require at least one read with these bases on \n");
    fprintf(file, "\t    either side of the indel[30]\n");
    fprintf(file, "\t-G, add genotype columns (FORMAT GT:AD:GQ) to the vcf output\n");
    fprintf(file, "\t-A, with indels.vcf: genotype the known indels in this sample\n");
    fprintf(file, "\t    (FORMAT GT:AD:GQ from the reads for and against each)\n");
    fprintf(file, "\t-P, with -G or -A: genotype PAIRED_READ records too, from the\n");
    fprintf(file, "\t    concordant pairs whose fragment spans the deletion\n");
    fprintf(file, "\t-D, with -G: depth evidence for deletions of 50 bp and more\n");
    fprintf(file, "\t    (FORMAT DM:DFC, median depth inside against the flanks)\n");
    fprintf(file, "\t-C, with -G: clipped-read breakpoints for the same deletions\n");
    fprintf(file, "\t    (FORMAT CB:CS, where soft-clipped reads pile up and how many)\n");
    fprintf(file, "\t-V, with -G -C: verify those breakpoints by the clipped bases\n");
    fprintf(file, "\t    (FORMAT CV:CH, reads that continue across the deletion, and the shift)\n");
    fprintf(file, "\t-I, with -G -C -V: write large insertions to this file, a VCF of its own\n");
    fprintf(file, "\t    (clipped reads from either side facing each other, and what they agree on)\n");
    fprintf(file, "\t-U, with -G -C -V: write tandem duplications to this file, a VCF of its own\n");
    fprintf(file, "\t    (clipped reads at its end that continue at its start; with -D their depth)\n");
    fprintf(file, "\t-N, with -G -C -V: write inversion breakpoints to this file, a VCF of its own\n");
    fprintf(file, "\t    (two piles of reads clipped on the same side that continue on the other strand at each other)\n");
    fprintf(file, "\t-M, with -U or -N: add PE= to their records, the read pairs whose orientation\n");
    fprintf(file, "\t    is the junction's (everted; both forward; both reverse) between two windows at the breakpoints\n");
    fprintf(file, "\t-T, with -G -C -V: write breakpoints between two contigs to this file, a VCF of its own\n");
    fprintf(file, "\t    (a pile of clipped reads on either contig that continue in the other, found through the read pairs that span them)\n");
    fprintf(file, "\t-S, with -U, -N or -T: add SR= to their records, the split reads (a soft-clipped\n");
    fprintf(file, "\t    primary record whose SA tag places the clipped part at the other breakpoint), from either end\n");
    fprintf(file, "\t-J, with -G: write the junctions the split reads name by themselves to this file, a VCF of its own\n");
    fprintf(file, "\t    (no clip pile and no verified bases needed: insertions at the junction, long micro-homology, scattered clips)\n");
    fprintf(file, "\t-K, with -J: genotype its junctions (FORMAT GT:AD:GQ:RB), the split reads against\n");
    fprintf(file, "\t    the reads that run through either end on the reference allele\n");
    fprintf(file, "\t-H, with -J: add HOMLEN, INSLEN and OA to its records, the micro-homology or the inserted bases\n");
    fprintf(file, "\t    that the split reads' own two alignments state, their median and how many reads agree on it\n");
    fprintf(file, "\t-E, with -J: add PE to its records, the read pairs on either side of the junction (for a deletion\n");
    fprintf(file, "\t    the pairs in the normal orientation that the aligner has not flagged as proper pairs)\n");
    fprintf(file, "\n");
    fprintf(file, "Assumptions:\n");
    fprintf(file, "\tThe BAM file is coordinate sorted\n");
    fprintf(file, "\tUnless specified in a config file, insertlengths for\n");
    fprintf(file, "\treadgroups, as well as average coverage per chromosome\n");
    fprintf(file, "\tare estimated from the BAM file (which can be slow!!!),\n");
    fprintf(file, "\tas well as lead to false negatives as some of the PE\n");
    fprintf(file, "\tevidence which is accounted for in one sample,might not\n");
    fprintf(file, "\tbe accounted for in the other\n");
}

static void free_range(void* p) { free(p); }

/* a keyed table that overflowed has answered nothing since; said once, at the end.  fmt takes the stored and the dropped count (%llu each) */
static void say_overflow(im_ctx* gpu, int (*stats)(im_ctx*, uint64_t*, uint64_t*), const char* fmt)
{
    uint64_t stored = 0, dropped = 0;
    if (stats(gpu, &stored, &dropped) == IM_OK && dropped > 0) fprintf(stderr, fmt, (unsigned long long)stored, (unsigned long long)dropped);
}

/* the evidence FILEs, in the order they are written on the pipelined path, and per contig on the record-at-a-time path (the same
 * genome-wide arrays and tables on both) */
static evfile g_evidence[3] = {
    {&g_ins_file, NULL, ins_describe, ins_contig, "large-insertion evidence (device)"},
    {&g_dup_file, NULL, dup_describe, dup_contig, "tandem-duplication evidence (device)"},
    {&g_inv_file, NULL, inv_describe, inv_contig, "inversion evidence (device)"},
};

int main(int argc, char** argv)
{
    t_is_main = 1;
    g_argv = xcalloc((size_t)argc + 1, sizeof(char*));          /* as given: the parsing below cuts the sample argument in two */
    for (int i = 0; i < argc; i++) g_argv[i] = xstrdup(argv[i]);
    {
        /* the record-at-a-time child of a pipeline run the reference aborts: its first bytes are on stdout already, and so is
         * everything it has to say on stderr until something goes wrong */
        const char* sk = getenv("INDELMINER_SKIP_STDOUT");
        const char* from = getenv("INDELMINER_HANDOFF_PARENT");       /* only the process that started this one may ask for it: a value
                                                                        * that leaked into somebody's environment drops nothing */
        if (sk && !(from && (long)getppid() == atol(from))) sk = NULL;
        if (sk) {
            g_out_skip = atoll(sk);
            unsetenv("INDELMINER_SKIP_STDOUT");
            t_out = out_cookie_open();
            if (getenv("INDELMINER_HANDOFF_QUIET") && !getenv("INDELMINER_DEBUG_HANDOFF")) {
                g_real_stderr = dup(STDERR_FILENO);
                if (!freopen("/dev/null", "w", stderr)) { }
            }
        }
    }
    O.maxdelsize = 1000; O.maxpedelsize = 1000000; O.minsupport = 2; O.klength = 6; O.numgaps = 0;
    O.outputformat = "vcf"; O.qthreshold = 10; O.ethreshold = 10; O.ethreshold_vcfcheck = 10;
    O.call_all_indels = 0; O.maxdiffsallowed = 6; O.minbalance = 30;
    const char* tie_env = getenv("INDELMINER_TIE_ORDER");       /* "expected": SURVEY.md 0.2 */
    O.tie_desc = (tie_env && strcmp(tie_env, "expected") == 0) ? 1 : 0;

    int c;
    while ((c = getopt(argc, argv, "dl:hc:e:o:k:g:x:i:s:p:tn:q:af:b:GAPDCVI:U:N:MT:SJ:KHE")) != -1) {
        switch (c) {
        case 'd': O.debug = 1; break;
        case 'l': break;
        case 'h': print_help(stdout); return EXIT_SUCCESS;
        case 'c': O.region = optarg; break;
        case 'e': if (sscanf(optarg, "%u", &O.minsupport) != 1) fatalf("incorrect option for -e: %s\n", optarg); break;
        case 'o': O.outputformat = optarg; break;
        case 'k': if (sscanf(optarg, "%u", &O.klength) != 1) fatalf("incorrect option for -k: %s\n", optarg); break;
        case 'f': if (sscanf(optarg, "%u", &O.maxdiffsallowed) != 1) fatalf("incorrect option for -f: %s\n", optarg); break;
        case 'g': if (sscanf(optarg, "%u", &O.numgaps) != 1) fatalf("incorrect option for -g: %s\n", optarg); break;
        case 'x': break;                                            /* accepted, unused (src/indelminer.c:793-794) */
        case 'i': O.configfile = optarg; break;
        case 's': if (sscanf(optarg, "%u", &O.maxdelsize) != 1) fatalf("incorrect option for -s: %s\n", optarg); break;
        case 'p': if (sscanf(optarg, "%u", &O.maxpedelsize) != 1) fatalf("incorrect option for -p: %s\n", optarg); break;
        case 't': break;                                            /* stored, never read (src/indelminer.c:775) */
        case 'n':
            if (sscanf(optarg, "%u", &O.ethreshold) != 1) fatalf("incorrect option for -n: %s\n", optarg);
            if (O.ethreshold < O.klength) O.ethreshold = O.klength;
            O.ethreshold_vcfcheck = O.ethreshold;
            break;
        case 'q': if (sscanf(optarg, "%d", &O.qthreshold) != 1) fatalf("incorrect option for -q: %s\n", optarg); break;
        case 'a': O.call_all_indels = 1; break;
        case 'b': if (sscanf(optarg, "%u", &O.minbalance) != 1) fatalf("incorrect option for -b: %s\n", optarg); break;
        case 'G': g_genotype = 1; break;                            /* not an option of the reference */
        case 'A': g_known_counts = 1; break;                        /* not an option of the reference */
        case 'P': g_pair_counts = 1; break;                         /* not an option of the reference */
        case 'D': g_depth_evidence = 1; break;                      /* not an option of the reference */
        case 'C': g_clip_evidence = 1; break;                       /* not an option of the reference */
        case 'V': g_clip_verify = 1; break;                         /* not an option of the reference */
        case 'I': g_ins_file = optarg; break;                       /* not an option of the reference */
        case 'U': g_dup_file = optarg; break;                       /* not an option of the reference */
        case 'N': g_inv_file = optarg; break;                       /* not an option of the reference */
        case 'M': g_pair_links = 1; break;                          /* not an option of the reference */
        case 'T': g_bnd_file = optarg; break;                       /* not an option of the reference */
        case 'S': g_split_links = 1; break;                         /* not an option of the reference */
        case 'J': g_junc_file = optarg; break;                      /* not an option of the reference */
        case 'K': g_junc_genotype = 1; break;                       /* not an option of the reference */
        case 'H': g_junc_overlap = 1; break;                        /* not an option of the reference */
        case 'E': g_junc_pairs = 1; break;                          /* not an option of the reference */
        case '?': break;
        default: print_help(stderr); return EXIT_FAILURE;
        }
    }
    forceassert(O.maxdelsize > 0);
    forceassert(O.klength > 1 && O.klength < 16);
    forceassert(strcmp(O.outputformat, "vcf") == 0 || strcmp(O.outputformat, "detailed") == 0);
    if (argc == optind) { print_help(stderr); return EXIT_FAILURE; }
    forceassert(argc - optind > 1);
    t0 = time(0);
    g_timing = getenv("INDELMINER_TIMING") != NULL;
    g_t_last = now_ms();

    const char* fasta_reference = argv[optind++];
    char* ptr = argv[optind++];
    if (g_known_counts && strchr(ptr, '=') != NULL) { fprintf(stderr, "indelminer: -A needs a VCF argument (annotate mode)\n"); return EXIT_FAILURE; }
    if (strchr(ptr, '=') == NULL) {                 /* a VCF: tag its indels only (src/indelminer.c:1046-1053) */
        g_vcfname = ptr;
        O.minsupport = 1;
        O.outputformat = "vcf";
        ptr = argv[optind++];
    }
    char* samplename = ptr;
    while (*ptr != '=') ptr++;
    *ptr = 0;
    const char* bam_name = ++ptr;
    g_sample_name = samplename;
    if (g_vcfname != NULL) O.ethreshold_vcfcheck = 0;   /* src/indelminer.c:1074 */
    if (g_genotype) {
        /* what -G does not do, said in one line */
        const char* ws_ = getenv("WORLD_SIZE");
        if (g_vcfname != NULL) { fprintf(stderr, "indelminer: -G is not available with a VCF argument (annotate mode)\n"); return EXIT_FAILURE; }
        if ((ws_ && atoi(ws_) > 1) || getenv("INDELMINER_FORCE_MGPU")) { fprintf(stderr, "indelminer: -G is not available with more than one rank\n"); return EXIT_FAILURE; }
    }

    if (g_known_counts) {
        const char* ws_ = getenv("WORLD_SIZE");
        if ((ws_ && atoi(ws_) > 1) || getenv("INDELMINER_FORCE_MGPU")) { fprintf(stderr, "indelminer: -A is not available with more than one rank\n"); return EXIT_FAILURE; }
    }

    /* -P: behind the refusals of -G and -A, in front of what the three need of the library (the newest entry points first) */
    if (g_pair_counts) {
        if (!g_genotype && !g_known_counts) { fprintf(stderr, "indelminer: -P needs -G or -A\n"); return EXIT_FAILURE; }
        if (!PAIR_API_PRESENT) {
            fprintf(stderr, "indelminer: genotyping paired-read records (-P) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -D: behind the refusals of -G, -A and -P; what it needs of the library in front of what -G needs (the newer entry points first) */
    if (g_depth_evidence) {
        if (g_vcfname != NULL) { fprintf(stderr, "indelminer: -D is not available with a VCF argument (annotate mode)\n"); return EXIT_FAILURE; }
        if (!g_genotype) { fprintf(stderr, "indelminer: -D needs -G\n"); return EXIT_FAILURE; }
        /* a region run builds no depth array, and the flanks would lie outside the walked stretch */
        if (O.region != NULL) { fprintf(stderr, "indelminer: -D is not available with -c\n"); return EXIT_FAILURE; }
        if (!MEDIAN_API_PRESENT) {
            fprintf(stderr, "indelminer: depth evidence (-D) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -C: behind the refusals of -G, -A, -P and -D, in the same order as -D's */
    if (g_clip_evidence) {
        if (g_vcfname != NULL) { fprintf(stderr, "indelminer: -C is not available with a VCF argument (annotate mode)\n"); return EXIT_FAILURE; }
        if (!g_genotype) { fprintf(stderr, "indelminer: -C needs -G\n"); return EXIT_FAILURE; }
        /* the slack, and the windows of a PAIRED_READ record, reach outside a walked stretch */
        if (O.region != NULL) { fprintf(stderr, "indelminer: -C is not available with -c\n"); return EXIT_FAILURE; }
        if (!CLIP_API_PRESENT) {
            fprintf(stderr, "indelminer: clip evidence (-C) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -V: behind -C's refusals; every other refusal reaches it through -G and -C */
    if (g_clip_verify) {
        if (!g_clip_evidence) { fprintf(stderr, "indelminer: -V needs -C\n"); return EXIT_FAILURE; }
        if (!CLIPTAIL_API_PRESENT) {
            fprintf(stderr, "indelminer: clip verification (-V) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -I: behind -V's refusals; every other refusal reaches it through -G, -C and -V */
    if (g_ins_file) {
        if (!g_clip_verify) { fprintf(stderr, "indelminer: -I needs -V\n"); return EXIT_FAILURE; }
        if (!FACING_API_PRESENT) {
            fprintf(stderr, "indelminer: large-insertion evidence (-I) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -U: behind -I's refusals, and independent of -I */
    if (g_dup_file) {
        if (!g_clip_verify) { fprintf(stderr, "indelminer: -U needs -V\n"); return EXIT_FAILURE; }
        if (!CROSSED_API_PRESENT) {
            fprintf(stderr, "indelminer: tandem-duplication evidence (-U) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -N: behind -I's and -U's refusals, and independent of both */
    if (g_inv_file) {
        if (!g_clip_verify) { fprintf(stderr, "indelminer: -N needs -V\n"); return EXIT_FAILURE; }
        if (!INVERTED_API_PRESENT) {
            fprintf(stderr, "indelminer: inversion evidence (-N) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -M: behind -N's refusals; every other refusal reaches it through -U or -N, that is through -G, -C and -V */
    if (g_pair_links) {
        if (!g_dup_file && !g_inv_file) { fprintf(stderr, "indelminer: -M needs -U or -N\n"); return EXIT_FAILURE; }
        if (!PAIRLINK_API_PRESENT) {
            fprintf(stderr, "indelminer: pair links (-M) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -T: behind -M's refusals, and independent of -I, -U, -N and -M */
    if (g_bnd_file) {
        if (!g_clip_verify) { fprintf(stderr, "indelminer: -T needs -V\n"); return EXIT_FAILURE; }
        if (!MATELINK_API_PRESENT) {
            fprintf(stderr, "indelminer: breakpoints between contigs (-T) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -S: behind -T's refusals; every other refusal reaches it through -U, -N or -T, that is through -G, -C and -V */
    if (g_split_links) {
        if (!g_dup_file && !g_inv_file && !g_bnd_file) { fprintf(stderr, "indelminer: -S needs -U, -N or -T\n"); return EXIT_FAILURE; }
        if (!SPLITLINK_API_PRESENT) {
            fprintf(stderr, "indelminer: split links (-S) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -J: behind -S's refusals; it needs -G alone (annotate mode and more than one rank are refused through it) and none of the others */
    if (g_junc_file) {
        if (!g_genotype) { fprintf(stderr, "indelminer: -J needs -G\n"); return EXIT_FAILURE; }
        /* a junction's far end, and the reads there that name it from the other side, lie outside a walked stretch */
        if (O.region != NULL) { fprintf(stderr, "indelminer: -J is not available with -c\n"); return EXIT_FAILURE; }
        if (!SPLITJUNC_API_PRESENT) {
            fprintf(stderr, "indelminer: split-link junctions (-J) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -K: behind -J's refusals; every other refusal reaches it through -J and -G */
    if (g_junc_genotype) {
        if (!g_junc_file) { fprintf(stderr, "indelminer: -K needs -J\n"); return EXIT_FAILURE; }
        if (!SPANENDS_API_PRESENT) {
            fprintf(stderr, "indelminer: junction genotypes (-K) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -H: behind -K's refusals; every other refusal reaches it through -J and -G */
    if (g_junc_overlap) {
        if (!g_junc_file) { fprintf(stderr, "indelminer: -H needs -J\n"); return EXIT_FAILURE; }
        if (!SPLITOVERLAP_API_PRESENT) {
            fprintf(stderr, "indelminer: junction overlap (-H) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    /* -E: behind -H's refusals; every other refusal reaches it through -J and -G */
    if (g_junc_pairs) {
        if (!g_junc_file) { fprintf(stderr, "indelminer: -E needs -J\n"); return EXIT_FAILURE; }
        if (!JUNCPAIR_API_PRESENT) {
            fprintf(stderr, "indelminer: junction pairs (-E) needs the device library\n"); return EXIT_FAILURE;
        }
    }
    if (g_genotype) {
        if (!SPAN_API_PRESENT) {
            fprintf(stderr, "indelminer: genotyping (-G) needs the device library\n"); return EXIT_FAILURE;
        }
        if (strcmp(O.outputformat, "detailed") == 0) { g_genotype = g_pair_counts = g_depth_evidence = g_clip_evidence = g_clip_verify = g_pair_links = g_split_links = g_junc_genotype = g_junc_overlap = g_junc_pairs = 0; g_ins_file = g_dup_file = g_inv_file = g_bnd_file = g_junc_file = NULL; }    /* -o detailed has no columns to add to, and builds no clip arrays to search */
    }
    if (g_known_counts) {
        if (!im_support_count || !SPAN_API_PRESENT) {
            fprintf(stderr, "indelminer: genotyping known indels (-A) needs the device library\n"); return EXIT_FAILURE;
        }
    }

    fprintf(stderr, "Reference fasta file: %s\n", fasta_reference);
    fprintf(stderr, "Chromosomal region  : %s\n", O.region == NULL ? "ALL" : O.region);
    fprintf(stderr, "BAM file            : %s\n", bam_name);
    if (g_vcfname != NULL) fprintf(stderr, "VCF file            : %s\n", g_vcfname);

    driver d;
    memset(&d, 0, sizeof d);
    d.depth_tid = -1;
    d.bam_name = bam_name;
    bgzf_reader* r = bgzf_open(bam_name);
    if (!r) fatalf("error in opening the file %s", bam_name);
    d.hdr = bam_header_load(r);
    if (!d.hdr) fatalf("%s is not a BAM file", bam_name);
    d.idx = bai_load(bam_name);
    if (!d.idx) fatalf("BAM indexing file is not available.");
    d.insertlengths = qhash_new(4);
    d.readpairs = qhash_new(20);

    int chromid = -1, chromstart = -1, chromstop = -1;
    if (O.region) bam_parse_region_str(d.hdr, O.region, &chromid, &chromstart, &chromstop);

    /* one process per GPU (torch.distributed.run's environment): contigs are sharded over the ranks */
    mgpu mg;
    memset(&mg, 0, sizeof mg);
    {
        const char* ws = getenv("WORLD_SIZE");
        const int world = ws ? atoi(ws) : 1;
        const char* pl = getenv("INDELMINER_PIPELINE");
        if ((world > 1 || getenv("INDELMINER_FORCE_MGPU")) && chromid == -1 && !(pl && strcmp(pl, "host") == 0)) {
            mg.world = world > 0 ? world : 1;
            mg.rank = getenv("RANK") ? atoi(getenv("RANK")) : 0;
            mg.local_rank = getenv("LOCAL_RANK") ? atoi(getenv("LOCAL_RANK")) : mg.rank;
            forceassert(mg.rank >= 0 && mg.rank < mg.world);
            g_mg = &mg; g_mg_rank = mg.rank; g_mg_local = mg.local_rank; g_mg_parts = 1;
            /* librccl prints a banner on descriptor 1: the VCF goes through part files and the saved descriptor, and
             * descriptor 1 points at stderr for the whole run */
            fflush(stdout);
            mg.out_fd = dup(1);
            if (mg.out_fd < 0 || dup2(2, 1) < 0) fatalf("cannot redirect stdout");
            mg.abort_tid = -1;
            if (g_vcfname != NULL) {
                /* annotate mode walks only the contigs the variant file names (src/indelminer.c:788) */
                mg.skip = xcalloc((size_t)d.hdr->n_targets, 1);
                for (int32_t i = 0; i < d.hdr->n_targets; i++) {
                    known_free(&g_known);
                    read_variants(g_vcfname, i, d.hdr->target_name[i], &g_known);
                    mg.skip[i] = g_known.n == 0;
                }
            }
            mg_plan(&mg, &d);                   /* before the walkers are planned: they take this rank's contigs */
        }
    }
    d.marker_floor = INT_MAX;

    /* the GPU: one context, opened by a helper thread while this thread reads the BAM (insert lengths) and the FASTA --
     * HIP start-up is 0.15-0.3 s of nothing but waiting */
    pthread_mutex_init(&d.gpu_mu, NULL); pthread_cond_init(&d.gpu_cv, NULL);
    d.gpu_pending = 1;
    if (pthread_create(&d.gpu_thread, NULL, gpu_open_thread, &d) != 0) fatalf("cannot start the GPU helper thread");
    /* the device pipeline: its walkers set their buffers up from now on.  A region run (-c) is the same pipeline over the pieces of
     * one stretch of one contig (its first piece also takes the records that reach into it from the front, as bam_fetch does;
     * mates outside the stretch and the depth around a variant are looked up in the file, like the reference does).
     * INDELMINER_PIPELINE=host is the record-at-a-time path, kept for runs the reference aborts (handoff_to_host_child). */
    walkpool_t* pool = NULL;
    {
        const char* pl0 = getenv("INDELMINER_PIPELINE");
        if (!(pl0 && strcmp(pl0, "host") == 0)) {
            if (chromid != -1) {
                g_region_tid = chromid; g_region_beg = chromstart; g_region_end = chromstop;
                /* not clipped to the contig's length: bam_fetch(tid, beg, end) with "ctg" alone means end = 2^29 and delivers records
                 * whose position lies behind the contig's end too (a whole-genome run, which fetches [0, length), never sees them) */
                if (g_region_end < g_region_beg) g_region_end = g_region_beg;
            }
            /* no config file: the insert lengths are estimated by the walk itself (run_pipeline) instead of by a pass of their own;
             * multi-GPU runs and annotate mode keep the pre-pass (the shard summaries / the serial walk need the table up front) */
            {
                const char* op = getenv("INDELMINER_ONEPASS");          /* INDELMINER_ONEPASS=0: the pre-pass of the reference's layout */
                /* several ranks: always the one walk (run_pipeline: the ranks exchange what their walks logged) */
                g_onepass = O.configfile == NULL && g_vcfname == NULL && chromid == -1 && (g_mg || !(op && strcmp(op, "0") == 0));
                if (PAIR_ON) g_onepass = 0;             /* -P: the first chunk's scatter looks read groups up in the finished table */
            }
            pool = walkpool_start(&d);
        }
    }
    if (g_mg) mg_rendezvous(&mg, &d);          /* the communicator comes up on a thread of its own, beside the FASTA read and the pre-walk */

    if (O.configfile) read_configuration(O.configfile, d.insertlengths, d.hdr);
    else if (g_onepass) { }
    else if (!g_mg) { if (chromid == -1 && pool && !getenv("INDELMINER_ESTIMATE_SERIAL")) estimate_insertlengths_threads(&d, pool->pieces, pool->n_pieces); else estimate_insertlengths(&d, chromid); }
    fprintf(stderr, "\nRead-group\tMin-value\tMax-value\n----------\t---------\t---------\n");
    for (uint32_t i = 0; i <= d.insertlengths->mask; i++)
        for (qbin* it = d.insertlengths->bins[i]; it; it = it->next)
            fprintf(stderr, "%s\t%d\t%d\n", it->name, ((int32_t*)it->val)[0], ((int32_t*)it->val)[1]);
    fprintf(stderr, "----------\t---------\t---------\n\n");
    if (!g_onepass && !(g_mg && O.configfile == NULL)) cov_print_table(d.hdr);      /* one-pass and multi-rank estimates: printed when every record has been seen */
    timestamp("Read insertlengths for the BAM file");
    phase_time("open BAM, index, insert lengths");

    const int nseq = fasta_load(fasta_reference, d.hdr->n_targets, &d.sequences, &d.seqlen, chromid);
    if (nseq < 0) fatalf("error in opening the file %s", fasta_reference);
    forceassert(nseq == d.hdr->n_targets);
    timestamp("Read the reference sequence");
    phase_time("read FASTA");

    /* the reference is in: the GPU helper (started before the insert-length pass) uploads it */
    pthread_mutex_lock(&d.gpu_mu);
    d.seq_ready = 1;
    pthread_cond_broadcast(&d.gpu_cv);
    pthread_mutex_unlock(&d.gpu_mu);


    const char* pl = getenv("INDELMINER_PIPELINE");
    const int use_pipeline = !(pl && strcmp(pl, "host") == 0);
    if (g_mg && pool->serial) {
        /* annotate mode: contigs are walked one by one behind each other's replays -- the logs come from a pass of their own */
        mg_exchange(&mg, &d, O.configfile == NULL, pool->pieces, pool->n_pieces, mg.piece_walker);
        mg_after_logs(&mg, &d);
    }
    if (use_pipeline) run_pipeline(&d, pool);
    if (g_mg) mg_finish(&mg, &d);
    /* the reference prints its header before it reads the first record (src/indelminer.c:745-754 in front of 756-): a run it
     * aborts on some record has the header on stdout.  Here the header waits for the GPU context (gpu_wait). */
    if (!use_pipeline) { gpu_wait(&d); evidence_enable(&d); }
    for (int32_t i = 0; i < d.hdr->n_targets && !use_pipeline; i++) {
        if (chromid != -1 && i != chromid) continue;
        if (g_vcfname != NULL) {
            known_free(&g_known);
            read_variants(g_vcfname, i, d.hdr->target_name[i], &g_known);
            if (g_known.n == 0) continue;           /* src/indelminer.c:788 */
        }
        if (chromid == -1) run_contig(&d, i, 0, d.hdr->target_len[i], r);
        else run_contig(&d, i, chromstart, chromstop, r);
        /* -I, -U, -N, record-at-a-time: behind the contig's flushes, on what its chunks scattered */
        for (int e = 0; e < 3; e++) if (*g_evidence[e].path) ev_contig(&g_evidence[e], &d, i);
    }

    gpu_wait(&d);
    for (int e = 0; e < 3; e++) {
        /* -I, then -U, then -N, pipelined: once, now that the last flush has printed and every scatter has completed; the genome-wide
         * arrays were never reset and the table is keyed by contig */
        if (!*g_evidence[e].path) continue;
        for (int32_t i = 0; i < d.hdr->n_targets && use_pipeline; i++) ev_contig(&g_evidence[e], &d, i);
        ev_finish(&g_evidence[e]);
    }
    /* -T: once, behind -N's FILE, on either path: a junction has its two piles on two contigs */
    if (MATELINK_ON) bnd_search(&d);
    /* -J: once, behind -T's FILE, on either path: the table is keyed by contig and holds every chunk's links by now */
    if (SPLITJUNC_ON) junc_search(&d);
    if (CLIPTAIL_ON) say_overflow(d.gpu, im_cliptail_stats, "indelminer: -V: the clip-tail table overflowed (%llu entries stored, %llu dropped): CV and CH are . from there on\n");
    if (PAIRLINK_ON) say_overflow(d.gpu, im_pairlink_stats, "indelminer: -M: the pair-link table overflowed (%llu links stored, %llu dropped): PE is . in the files of -U and -N\n");
    if (MATELINK_ON) say_overflow(d.gpu, im_matelink_stats, "indelminer: -T: the mate-link table overflowed (%llu links stored, %llu dropped): its file has no records\n");
    if (SPLITLINK_ON) say_overflow(d.gpu, im_splitlink_stats, "indelminer: -S: the split-link table overflowed (%llu links stored, %llu dropped): SR is . in the files of -U, -N and -T\n");
    if (SPLITJUNC_ON) say_overflow(d.gpu, im_splitlink_stats, "indelminer: -J: the split-link table overflowed (%llu links stored, %llu dropped): its file has no records\n");
    if (JUNCPAIR_ON) say_overflow(d.gpu, im_pairlink_stats, "indelminer: -E: the pair-link table overflowed (%llu links stored, %llu dropped): PE is . on one contig in the file of -J\n");
    if (JUNCPAIR_ON) say_overflow(d.gpu, im_matelink_stats, "indelminer: -E: the mate-link table overflowed (%llu links stored, %llu dropped): PE is .,. on two contigs in the file of -J\n");
    if (t_out) fflush(t_out);
    if (g_timing) fprintf(stderr, "[timing] DP=: %ld windows asked of the device, %ld of them answered from the file (a position of %d records or more within %d bases in front)\n",
                          (long)g_dp_queries, (long)g_dp_from_file, DP_DEEP_LOCUS, (int)g_longest_span);
    if (g_vcfname != NULL) cpu_report();            /* annotate mode has no replay workers: its report comes here */
    if (!getenv("INDELMINER_TIDY_EXIT")) {
        /* everything is printed: the GPU context, the pinned rings and the device arrays go with the process -- tearing the
         * HIP runtime down in order costs about as long as the whole device work of a small run (leak checkers: INDELMINER_TIDY_EXIT=1) */
        fflush(stdout);
        phase_time("output flushed; the process ends (what follows is the kernel taking it apart)");
        fflush(stderr);
        _exit(EXIT_SUCCESS);
    }
    im_ctx_destroy(d.gpu);
    bgzf_close(r);
    bai_free(d.idx);
    qhash_free(d.insertlengths, free_range);
    return EXIT_SUCCESS;
}
