"""One batch of host-prepared candidate reads resident on the device, as the realign probes in this directory launch it
(im_dev_realign alone; not part of bench.py or the product)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from indelminer_amd import capi  # noqa: E402


class CandBatch:
    def __init__(self, ctx, cand, read_len):
        self.ctx = ctx
        n = self.n = len(cand["index"])
        stride = (read_len + 3) // 4 * 4
        bases = np.zeros((n, stride), dtype=np.uint8)
        bases[:, :read_len] = cand["bases"]
        flat = np.concatenate([bases.reshape(-1), np.zeros(16, np.uint8)])
        self.bufs = [capi.DevBuf(ctx, flat.nbytes).upload(flat),
                     capi.DevBuf(ctx, 8 * n).upload(np.arange(n, dtype=np.int64) * stride),
                     capi.DevBuf(ctx, 4 * n).upload(np.full(n, read_len, np.int32)),
                     capi.DevBuf(ctx, 4 * n).upload(np.zeros(n, np.int32)),
                     capi.DevBuf(ctx, 4 * n).upload(cand["anchor"].astype(np.int32)),
                     capi.DevBuf(ctx, 4 * n).upload(cand["range_max"].astype(np.int32))]
        self.d_res = capi.DevBuf(ctx, 512 * n)
        self.batch = capi.DevBatch(n, *(b.ptr for b in self.bufs), self.d_res.ptr, None, None, None)
        self.P = capi.params()

    def realign(self):
        self.ctx._check(capi.lib().im_dev_realign(self.ctx.h, C.byref(self.P), C.byref(self.batch), self.ctx.stream))

    def sync(self):
        self.ctx._check(capi.lib().im_stream_sync(self.ctx.h, self.ctx.stream))

    def results(self):
        return self.d_res.download(capi.RESULT_DTYPE, self.n)
