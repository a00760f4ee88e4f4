/* The seven entry points of -T as stubs that fail: linked beside im_shim.c, clip_entries_stub.c, cliptail_entries_stub.c,
 * facing_entries_stub.c, crossed_entries_stub.c, inverted_entries_stub.c and pairlink_entries_stub.c they make a library that has
 * -C's, -V's, -I's, -U's, -N's, -M's and -T's entries and lacks -S's, which is what tests/test_splitlink_host.py needs to reach -S's
 * own refusal.  TEST INFRASTRUCTURE; nothing calls them, the driver refuses before it opens a context. */
#include "indelminer_amd.h"

int im_matelink_enable(im_ctx* ctx, int32_t min_mapq, int32_t log2_slots)
{
    (void)ctx; (void)min_mapq; (void)log2_slots;
    return IM_E_ARG;
}
int im_dev_matelink_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream)
{
    (void)ctx; (void)recs; (void)stream;
    return IM_E_ARG;
}
int im_matelink_add(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* pos, const int32_t* mtid, const int32_t* mpos, const uint8_t* kind)
{
    (void)ctx; (void)tid; (void)n; (void)pos; (void)mtid; (void)mpos; (void)kind;
    return IM_E_ARG;
}
int im_matelink_partner(im_ctx* ctx, int32_t tid, int32_t nq, const uint8_t* kind, const int32_t* a0, const int32_t* a1, uint32_t* n_links,
                        int32_t* mtid_out, uint32_t* n_partner, int32_t* lo, int32_t* hi)
{
    (void)ctx; (void)tid; (void)nq; (void)kind; (void)a0; (void)a1; (void)n_links; (void)mtid_out; (void)n_partner; (void)lo; (void)hi;
    return IM_E_ARG;
}
int im_matelink_reset(im_ctx* ctx, void* stream)
{
    (void)ctx; (void)stream;
    return IM_E_ARG;
}
int im_matelink_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped)
{
    (void)ctx; (void)stored; (void)dropped;
    return IM_E_ARG;
}
int im_cliptail_junction(im_ctx* ctx, int32_t nq, const int32_t* tid1, const int32_t* p1, const uint8_t* side1, const int32_t* tid2, const int32_t* p2,
                         const uint8_t* side2, int32_t max_shift, uint32_t* v1, uint32_t* v2, int32_t* shift, uint32_t* stored1, uint32_t* stored2)
{
    (void)ctx; (void)nq; (void)tid1; (void)p1; (void)side1; (void)tid2; (void)p2; (void)side2; (void)max_shift; (void)v1; (void)v2; (void)shift;
    (void)stored1; (void)stored2;
    return IM_E_ARG;
}
