/* The six clip-tail entry points of -V as stubs that fail: linked beside im_shim.c and clip_entries_stub.c they make a library that
 * has -C's and -V's entries and lacks -I's, which is what tests/test_facing_host.py needs to reach -I's own refusal.
 * TEST INFRASTRUCTURE; nothing calls them, the driver refuses before it opens a context. */
#include "indelminer_amd.h"

int im_cliptail_enable(im_ctx* ctx, int32_t min_clip, int32_t min_mapq, int32_t log2_slots) { (void)ctx; (void)min_clip; (void)min_mapq; (void)log2_slots; return IM_E_ARG; }
int im_dev_cliptail_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream) { (void)ctx; (void)recs; (void)stream; return IM_E_ARG; }
int im_cliptail_add(im_ctx* ctx, int32_t tid, int32_t n, const int32_t* pos, const uint8_t* side, const uint8_t* nbases, const uint32_t* planes)
{ (void)ctx; (void)tid; (void)n; (void)pos; (void)side; (void)nbases; (void)planes; return IM_E_ARG; }
int im_cliptail_verify(im_ctx* ctx, int32_t tid, int32_t nq, const int32_t* pr, const int32_t* pl, int32_t max_shift, uint32_t* v_right,
                       uint32_t* v_left, int32_t* shift, uint32_t* stored_right, uint32_t* stored_left)
{ (void)ctx; (void)tid; (void)nq; (void)pr; (void)pl; (void)max_shift; (void)v_right; (void)v_left; (void)shift; (void)stored_right; (void)stored_left; return IM_E_ARG; }
int im_cliptail_reset(im_ctx* ctx, void* stream) { (void)ctx; (void)stream; return IM_E_ARG; }
int im_cliptail_stats(im_ctx* ctx, uint64_t* stored, uint64_t* dropped) { (void)ctx; (void)stored; (void)dropped; return IM_E_ARG; }
