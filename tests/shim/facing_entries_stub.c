/* The three entry points of -I as stubs that fail: linked beside im_shim.c, clip_entries_stub.c and cliptail_entries_stub.c they make a
 * library that has -C's, -V's and -I's entries and lacks -U's, which is what tests/test_crossed_host.py needs to reach -U's own refusal.
 * TEST INFRASTRUCTURE; nothing calls them, the driver refuses before it opens a context. */
#include "indelminer_amd.h"

int im_clip_facing_tid(im_ctx* ctx, int32_t tid, int32_t min_reads, int32_t max_overlap, int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr,
                       uint32_t* cl, int32_t* n_found)
{ (void)ctx; (void)tid; (void)min_reads; (void)max_overlap; (void)cap; (void)pr; (void)pl; (void)cr; (void)cl; (void)n_found; return IM_E_ARG; }
int im_clip_facing(im_ctx* ctx, int32_t min_reads, int32_t max_overlap, int32_t cap, int32_t* pr, int32_t* pl, uint32_t* cr, uint32_t* cl,
                   int32_t* n_found)
{ (void)ctx; (void)min_reads; (void)max_overlap; (void)cap; (void)pr; (void)pl; (void)cr; (void)cl; (void)n_found; return IM_E_ARG; }
int im_cliptail_consensus(im_ctx* ctx, int32_t tid, int32_t nq, const int32_t* pos, const uint8_t* side, int32_t min_cover, uint32_t* entries,
                          uint32_t* len, uint32_t* planes, uint32_t* agree)
{ (void)ctx; (void)tid; (void)nq; (void)pos; (void)side; (void)min_cover; (void)entries; (void)len; (void)planes; (void)agree; return IM_E_ARG; }
