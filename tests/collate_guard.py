"""What tests/test_collate_gpu.py, tests/test_pretrain_collate_gpu.py and tests/test_mrc_collate_gpu.py share: outputs inside
guard bands, pre-filled with a sentinel byte, and the upload of a numpy dataset (test infrastructure)."""
import numpy as np
import torch

GUARD, GUARD_BYTE, SENTINEL_BYTE = 256, 0x5A, 0xCD      # GUARD % 16 == 0: img_feat / feat_targets stay 16-byte aligned behind the band


def to_device(a):
    return {k: (None if v is None else torch.from_numpy(v).cuda()) for k, v in a.items()}


class Guarded(object):
    """an output tensor inside a larger byte buffer: [guard | extent, filled with `fill` | guard]"""

    def __init__(self, shape, dtype, fill=SENTINEL_BYTE):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.nbytes, self.fill = n, fill
        self.buf = torch.full((GUARD + n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device='cuda')
        self.buf[GUARD:GUARD + n] = fill
        self.t = self.buf[GUARD:GUARD + n].view(dtype).view(shape)

    def check_guards(self, what):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == GUARD_BYTE).all()) and bool((b[GUARD + self.nbytes:] == GUARD_BYTE).all()), '%s: a guard byte changed' % what

    def untouched(self, first_byte=0):
        return bool((self.buf[GUARD + first_byte:GUARD + self.nbytes] == self.fill).all())


def sentinel_of(dtype):
    return torch.full((1,), SENTINEL_BYTE, dtype=torch.uint8).repeat(8).view(dtype)[0]
