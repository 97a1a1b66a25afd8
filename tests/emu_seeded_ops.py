"""tc_randn_clips on the emulated operator contract: the numpy restatement (tests/philox_ref.py) rounded to fp32, and a log
of every draw asked for, so that the samplers' seeded host logic runs -- and can be audited -- without a GPU
(tests/test_seeded_noise_cpu.py)."""
import numpy as np
import torch

import philox_ref
from emu_pinned_ops import EmuPinnedOps


class EmuSeededOps(EmuPinnedOps):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.draws = []                      # (seeds, shape, stream, scale) of every randn_clips call, in order

    def randn_clips(self, seeds, shape, stream, scale=1.0, out=None, raw=False):
        assert all(type(s) is int and 0 <= s < 1 << 64 for s in seeds), "the sampler hands over checked Python ints"
        shape = tuple(int(v) for v in shape)
        assert len(seeds) == shape[0]
        self.draws.append((tuple(seeds), shape, int(stream), float(scale)))
        n = int(np.prod(shape[1:], dtype=np.int64))
        if raw:
            res = torch.from_numpy(np.stack([philox_ref.words(s, n, stream) for s in seeds]).view(np.int32).reshape(shape))
        else:
            z = philox_ref.rows(seeds, n, stream).astype(np.float32) * np.float32(scale)
            res = torch.from_numpy(z.reshape(shape))
        if out is None:
            return res
        out.copy_(res)
        return out
