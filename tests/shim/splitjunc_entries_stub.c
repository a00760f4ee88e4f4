/* The entry points of -S, -J, -K and -H as stubs that fail: linked beside im_shim.c, pairlink_entries_stub.c and matelink_entries_stub.c
 * they make a library that has the pair links', the mate links', the split links', the junctions', the junction genotypes' and the
 * junction overlap's entries and lacks im_pairlink_stretched_enable and im_junction_pairs, which is what
 * tests/test_junction_pairs_host.py needs to reach -E's own refusal.  TEST INFRASTRUCTURE; nothing calls them, the driver refuses
 * before it opens a context. */
#include "indelminer_amd.h"

int im_splitlink_enable(im_ctx* ctx, int32_t min_clip, int32_t min_mapq, int32_t log2_slots, int32_t n_names, const char* const* names)
{
    (void)ctx; (void)min_clip; (void)min_mapq; (void)log2_slots; (void)n_names; (void)names;
    return IM_E_ARG;
}
int im_dev_splitlink_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream)
{
    (void)ctx; (void)recs; (void)stream;
    return IM_E_ARG;
}
int im_splitlink_add(im_ctx* ctx, int32_t n, const int32_t* tid, const int32_t* pos, const uint8_t* side, const int32_t* tid2, const int32_t* pos2,
                     const uint8_t* side2)
{
    (void)ctx; (void)n; (void)tid; (void)pos; (void)side; (void)tid2; (void)pos2; (void)side2;
    return IM_E_ARG;
}
int im_splitlink_count(im_ctx* ctx, int32_t nq, const int32_t* tid1, const uint8_t* side1, const int32_t* a0, const int32_t* a1,
                       const int32_t* tid2, const uint8_t* side2, const int32_t* b0, const int32_t* b1, uint32_t* count_out)
{
    (void)ctx; (void)nq; (void)tid1; (void)side1; (void)a0; (void)a1; (void)tid2; (void)side2; (void)b0; (void)b1; (void)count_out;
    return IM_E_ARG;
}
int im_splitlink_reset(im_ctx* ctx, void* stream)
{
    (void)ctx; (void)stream;
    return IM_E_ARG;
}
int im_splitlink_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped)
{
    (void)ctx; (void)stored; (void)dropped;
    return IM_E_ARG;
}
int im_splitlink_junctions(im_ctx* ctx, int32_t window, int32_t min_links, int32_t min_span, int32_t cap, int32_t* tid1, int32_t* pos1, uint8_t* side1,
                           int32_t* tid2, int32_t* pos2, uint8_t* side2, uint32_t* exact, uint32_t* n1, uint32_t* n2, int32_t* found)
{
    (void)ctx; (void)window; (void)min_links; (void)min_span; (void)cap; (void)tid1; (void)pos1; (void)side1; (void)tid2; (void)pos2; (void)side2;
    (void)exact; (void)n1; (void)n2; (void)found;
    return IM_E_ARG;
}
int im_span_query_ends(im_ctx* ctx, int32_t n, const int32_t* tid, const int32_t* pos, int32_t slack, uint32_t* min_out)
{
    (void)ctx; (void)n; (void)tid; (void)pos; (void)slack; (void)min_out;
    return IM_E_ARG;
}
int im_splitlink_overlap_enable(im_ctx* ctx)
{
    (void)ctx;
    return IM_E_ARG;
}
int im_splitlink_add_overlap(im_ctx* ctx, int32_t n, const int32_t* tid, const int32_t* pos, const uint8_t* side, const int32_t* tid2, const int32_t* pos2,
                             const uint8_t* side2, const int16_t* d)
{
    (void)ctx; (void)n; (void)tid; (void)pos; (void)side; (void)tid2; (void)pos2; (void)side2; (void)d;
    return IM_E_ARG;
}
int im_splitlink_overlap(im_ctx* ctx, int32_t n, const int32_t* tid1, const int32_t* pos1, const uint8_t* side1, const int32_t* tid2, const int32_t* pos2,
                         const uint8_t* side2, int32_t window, uint32_t* known, int32_t* median, uint32_t* agree)
{
    (void)ctx; (void)n; (void)tid1; (void)pos1; (void)side1; (void)tid2; (void)pos2; (void)side2; (void)window; (void)known; (void)median; (void)agree;
    return IM_E_ARG;
}
