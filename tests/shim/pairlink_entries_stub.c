/* The six entry points of -M as stubs that fail: linked beside im_shim.c, clip_entries_stub.c, cliptail_entries_stub.c,
 * facing_entries_stub.c, crossed_entries_stub.c and inverted_entries_stub.c they make a library that has -C's, -V's, -I's, -U's, -N's
 * and -M's entries and lacks -T's, which is what tests/test_intercontig_host.py needs to reach -T's own refusal.  TEST INFRASTRUCTURE;
 * nothing calls them, the driver refuses before it opens a context. */
#include "indelminer_amd.h"

int im_pairlink_enable(im_ctx* ctx, int32_t min_mapq, int32_t log2_slots)
{
    (void)ctx; (void)min_mapq; (void)log2_slots;
    return IM_E_ARG;
}
int im_dev_pairlink_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream)
{
    (void)ctx; (void)recs; (void)stream;
    return IM_E_ARG;
}
int im_pairlink_add(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* pos, const int32_t* mpos, const uint8_t* kind)
{
    (void)ctx; (void)tid; (void)n; (void)pos; (void)mpos; (void)kind;
    return IM_E_ARG;
}
int im_pairlink_count(im_ctx* ctx, int32_t tid, int32_t nq, const uint8_t* kind, const int32_t* a0, const int32_t* a1, const int32_t* b0,
                      const int32_t* b1, int32_t min_sep, uint32_t* count_out)
{
    (void)ctx; (void)tid; (void)nq; (void)kind; (void)a0; (void)a1; (void)b0; (void)b1; (void)min_sep; (void)count_out;
    return IM_E_ARG;
}
int im_pairlink_reset(im_ctx* ctx, void* stream)
{
    (void)ctx; (void)stream;
    return IM_E_ARG;
}
int im_pairlink_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped)
{
    (void)ctx; (void)stored; (void)dropped;
    return IM_E_ARG;
}
