"""The device rig of the plan tests (tests/test_gpu_cols_plan.py, tests/test_gpu_lane8_plan.py): every test under a limit of
its own, the caller's outputs cut from one arena between guard zones and filled with a sentinel before every launch, a few
distinct pairs replicated to a launch's pair count on the device."""
import faulthandler

import numpy as np
import pytest

LIMIT_S = 120
GUARD, SENTINEL = 4096, 0xA5


@pytest.fixture(autouse=True)
def time_limit():
    """Every test's device work under a limit of its own.  The exit is deliberate: a step that hangs on the device ends
    the whole process at once (os._exit behind a traceback), so that nothing more is started on a card that hung -- the
    tests behind it go without a report, which is the lesser evil.  Each test runs a few seconds; the limit is far above
    that and only a hang reaches it."""
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def tiled(torch, arr, n, device):
    """The first n of the endlessly repeated frames: pair i holds content i % k."""
    t = torch.from_numpy(arr).to(device)
    return t.repeat((-(-n // t.shape[0]), 1, 1))[:n]


class Arena:
    """blocks, subdirs, flows and the workspace between guard zones of one allocation."""

    def __init__(self, torch, device, n, nb, ws_bytes):
        sizes = dict(blocks=4 * n * nb, subdirs=n * nb, flows=16 * n, ws=ws_bytes)
        total = sum(GUARD + (v + 255) // 256 * 256 for v in sizes.values()) + GUARD
        self.mem = torch.empty((total,), dtype=torch.uint8, device=device)
        self.views, self.at, self.gaps = {}, {}, [(0, GUARD)]
        off = GUARD
        for k, v in sizes.items():
            self.views[k], self.at[k] = self.mem[off:off + v], (off, off + v)
            end = off + (v + 255) // 256 * 256
            self.gaps.append((off + v, end + GUARD))
            off = end + GUARD
        self.n, self.nb = n, nb
        assert self.views["ws"].data_ptr() % 256 == 0 and self.views["blocks"].data_ptr() % 4 == 0

    def refill(self):
        self.mem.fill_(SENTINEL)

    def args(self, torch, subpixel):
        return dict(blocks=self.views["blocks"].view(torch.int32).view(self.n, self.nb),
                    subdirs=self.views["subdirs"].view(self.n, self.nb) if subpixel else None,
                    flows=self.views["flows"].view(self.n, 16), workspace=self.views["ws"])

    def outputs(self):
        """The three outputs and whether every guard zone still holds the sentinel (the workspace itself is not read back)."""
        ws_lo, ws_hi = self.at["ws"]
        head, tail = self.mem[:ws_lo].cpu().numpy(), self.mem[ws_hi:].cpu().numpy()
        for lo, hi in self.gaps:
            zone = head[lo:min(hi, ws_lo)] if lo < ws_lo else tail[lo - ws_hi:hi - ws_hi]
            assert (zone == SENTINEL).all(), ("guard zone written", lo, hi, np.flatnonzero(zone != SENTINEL)[:8])
        cut = lambda k: head[self.at[k][0]:self.at[k][1]]
        return cut("blocks").view(np.uint32).reshape(self.n, self.nb), cut("subdirs").reshape(self.n, self.nb), cut("flows").reshape(self.n, 16)
