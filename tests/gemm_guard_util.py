"""Guarded GPU storage of the kernel-level GEMM tests (tests/test_gemm_epi_kernels_gpu.py,
tests/test_gemm_map_kernels_gpu.py): an output window inside a larger block, compared bit for bit
with its contents before the call everywhere the call must not write."""
import torch

NAN = float("nan")
ROW0 = 4            # the window's first row in its block


def _bits(t):
    return t.contiguous().view(torch.int32)


class Block:
    """An [m, n] window inside a NaN-filled block of m + 8 rows, `ld` apart, at row 4 and column `col`.
    fill: the window on entry; margin: what the rest of the block holds instead of NaN ([m + 8, ld];
    a stray atomic add into NaN would leave the bits unchanged, into a finite value it does not)."""

    def __init__(self, m, n, ld, col, fill=None, margin=None):
        host = torch.full((m + 8, ld), NAN) if margin is None else margin.clone()
        if fill is not None:
            host[ROW0:ROW0 + m, col:col + n] = fill
        self.m, self.n, self.col = m, n, col
        self.dev = host.cuda()
        self.before = _bits(host)
        self.win = self.dev[ROW0:ROW0 + m, col:col + n]

    def check(self, live, name):
        """Everything but the first `live` rows of the window bit-identical to before; returns those rows."""
        touched = torch.zeros(self.m, self.n, dtype=torch.bool)
        touched[:live] = True
        return self.check_touched(touched, name)[:live]

    def check_touched(self, touched, name):
        """Everything but the window's elements under the mask `touched` [m, n] bit-identical to before;
        returns the window."""
        after = self.dev.cpu()
        keep = torch.ones(after.shape, dtype=torch.bool)
        keep[ROW0:ROW0 + self.m, self.col:self.col + self.n] = ~touched
        changed = (_bits(after) != self.before) & keep
        assert not changed.any(), "%s: %d elements outside the live window changed, first at %s" % (
            name, int(changed.sum()), changed.nonzero()[0].tolist())
        return after[ROW0:ROW0 + self.m, self.col:self.col + self.n]
