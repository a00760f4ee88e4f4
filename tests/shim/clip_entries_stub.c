/* The six clip entry points of -C as stubs that fail: linked beside im_shim.c they make a library that has -C's entries and lacks
 * -V's, which is what tests/test_cliptail_host.py needs to reach -V's own refusal.  TEST INFRASTRUCTURE; nothing calls them, the
 * driver refuses before it opens a context. */
#include "indelminer_amd.h"

int im_clip_enable(im_ctx* ctx, int32_t min_clip, int32_t min_mapq) { (void)ctx; (void)min_clip; (void)min_mapq; return IM_E_ARG; }
int im_dev_clip_scatter(im_ctx* ctx, const im_dev_records* recs, void* stream) { (void)ctx; (void)recs; (void)stream; return IM_E_ARG; }
int im_clip_reset(im_ctx* ctx, int32_t tid, void* stream) { (void)ctx; (void)tid; (void)stream; return IM_E_ARG; }
int im_clip_query_tid(im_ctx* ctx, int32_t tid, int32_t n, const uint8_t* side, const int32_t* beg, const int32_t* end, uint32_t* count_out, int32_t* pos_out)
{ (void)ctx; (void)tid; (void)n; (void)side; (void)beg; (void)end; (void)count_out; (void)pos_out; return IM_E_ARG; }
int im_clip_build(im_ctx* ctx, int64_t contig_len, int32_t n, const int32_t* pos, const uint8_t* side) { (void)ctx; (void)contig_len; (void)n; (void)pos; (void)side; return IM_E_ARG; }
int im_clip_query(im_ctx* ctx, int32_t n, const uint8_t* side, const int32_t* beg, const int32_t* end, uint32_t* count_out, int32_t* pos_out)
{ (void)ctx; (void)n; (void)side; (void)beg; (void)end; (void)count_out; (void)pos_out; return IM_E_ARG; }
