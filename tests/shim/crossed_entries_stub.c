/* The four entry points of -U as stubs that fail: linked beside im_shim.c, clip_entries_stub.c, cliptail_entries_stub.c and
 * facing_entries_stub.c they make a library that has -C's, -V's, -I's and -U's entries and lacks -N's, which is what
 * tests/test_inverted_host.py needs to reach -N's own refusal.  TEST INFRASTRUCTURE; nothing calls them, the driver refuses before it
 * opens a context. */
#include "indelminer_amd.h"

int im_clip_peaks_tid(im_ctx* ctx, int32_t tid, int32_t side, int32_t min_reads, int32_t reach, int32_t cap, int32_t* pos, uint32_t* count,
                      int32_t* n_found)
{ (void)ctx; (void)tid; (void)side; (void)min_reads; (void)reach; (void)cap; (void)pos; (void)count; (void)n_found; return IM_E_ARG; }
int im_clip_peaks(im_ctx* ctx, int32_t side, int32_t min_reads, int32_t reach, int32_t cap, int32_t* pos, uint32_t* count, int32_t* n_found)
{ (void)ctx; (void)side; (void)min_reads; (void)reach; (void)cap; (void)pos; (void)count; (void)n_found; return IM_E_ARG; }
int im_clip_crossed_tid(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift,
                        int32_t min_verified, int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr, uint32_t* cl, uint32_t* v_right, uint32_t* v_left,
                        int32_t* shift, uint32_t* stored_right, uint32_t* stored_left, int32_t* n_found)
{
    (void)ctx; (void)tid; (void)min_reads; (void)reach; (void)min_len; (void)max_len; (void)max_shift; (void)min_verified; (void)cap; (void)pr; (void)pl;
    (void)cr; (void)cl; (void)v_right; (void)v_left; (void)shift; (void)stored_right; (void)stored_left; (void)n_found;
    return IM_E_ARG;
}
int im_clip_crossed(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t reach, int32_t min_len, int32_t max_len, int32_t max_shift,
                    int32_t min_verified, int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr, uint32_t* cl, uint32_t* v_right, uint32_t* v_left,
                    int32_t* shift, uint32_t* stored_right, uint32_t* stored_left, int32_t* n_found)
{
    (void)ctx; (void)tid; (void)min_reads; (void)reach; (void)min_len; (void)max_len; (void)max_shift; (void)min_verified; (void)cap; (void)pr; (void)pl;
    (void)cr; (void)cl; (void)v_right; (void)v_left; (void)shift; (void)stored_right; (void)stored_left; (void)n_found;
    return IM_E_ARG;
}
