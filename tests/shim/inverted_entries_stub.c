/* The two entry points of -N as stubs that fail: linked beside im_shim.c, clip_entries_stub.c, cliptail_entries_stub.c,
 * facing_entries_stub.c and crossed_entries_stub.c they make a library that has -C's, -V's, -I's, -U's and -N's entries and lacks
 * -M's, which is what tests/test_pairlink_host.py needs to reach -M's own refusal.  TEST INFRASTRUCTURE; nothing calls them, the driver
 * refuses before it opens a context. */
#include "indelminer_amd.h"

int im_clip_inverted_tid(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift,
                         int32_t min_verified, int32_t cap, uint8_t* side, int32_t* p1, int32_t* p2, uint32_t* c1, uint32_t* c2, uint32_t* v1,
                         uint32_t* v2, int32_t* shift, uint32_t* stored1, uint32_t* stored2, int32_t* n_found)
{
    (void)ctx; (void)tid; (void)min_reads; (void)reach; (void)min_len; (void)max_len; (void)max_shift; (void)min_verified; (void)cap; (void)side;
    (void)p1; (void)p2; (void)c1; (void)c2; (void)v1; (void)v2; (void)shift; (void)stored1; (void)stored2; (void)n_found;
    return IM_E_ARG;
}
int im_clip_inverted(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift,
                     int32_t min_verified, int32_t cap, uint8_t* side, int32_t* p1, int32_t* p2, uint32_t* c1, uint32_t* c2, uint32_t* v1,
                     uint32_t* v2, int32_t* shift, uint32_t* stored1, uint32_t* stored2, int32_t* n_found)
{
    (void)ctx; (void)tid; (void)min_reads; (void)reach; (void)min_len; (void)max_len; (void)max_shift; (void)min_verified; (void)cap; (void)side;
    (void)p1; (void)p2; (void)c1; (void)c2; (void)v1; (void)v2; (void)shift; (void)stored1; (void)stored2; (void)n_found;
    return IM_E_ARG;
}
