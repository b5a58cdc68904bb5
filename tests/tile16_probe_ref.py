"""Host model of the 16x16 adaptive search's probe (k_tile16_probe in k_search_tile16.hip, with the sample strides its
launcher chooses), in plain int64 numpy (tests only).

It restates the rules of the kernel's comments and DESIGN.md ("k_tile16_probe"), not its packed-u16 code, and returns the
whole word the probe writes into aof_ws_layout.hints: verdict | separation << 8.

    verdict 0  the exhaustive scan            2  step A on one-row bounds (tile row 4)
            1  step A on two-row bounds       3  ... on four-row bounds     4  ... on eight-row bounds

The constants carry the kernel's names, so that a retune changes both in one commit."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

K_SIDE = 17                          # kSide: 2S + 1 candidates per axis
K_BOUND_ROWS = 2                     # kBoundRows
K_PROBE_STRIDE = 8                   # kProbeStride
K_PROBE_MAX_BLOCKS = 128             # kProbeMaxBlocks
K_FULL_OVER_BOUND = 6                # kFullOverBound
K_MAX_SURVIVORS_PCT = 35             # kMaxSurvivorsPct
K_FULL_OVER_ONE_ROW = 12             # kFullOverOneRow
K_MAX_ONE_ROW_SURVIVORS_PCT = 4      # kMaxOneRowSurvivorsPct
K_MAX_FOUR_ROW_SURVIVORS_PCT = 40    # kMaxFourRowSurvivorsPct
K_MAX_EIGHT_ROW_SURVIVORS_PCT = 10   # kMaxEightRowSurvivorsPct
K_MAX_SEPARATION_FOR_DEEPER_LOOK = 450   # kMaxSeparationForDeeperLook

TILE = 16
# tile rows each bound sums: the two-row bound takes rows 8/kBoundRows + k*16/kBoundRows, the one-row bound the first of them
TWO_ROWS = tuple(range(8 // K_BOUND_ROWS, TILE, TILE // K_BOUND_ROWS))   # (4, 12)
ONE_ROW = TWO_ROWS[:1]                                                  # (4,)
FOUR_ROWS = (2, 6, 10, 14)
EIGHT_ROWS = tuple(range(0, TILE, 2))                                   # 0, 2, .., 14


def probe_samples(n, stride):
    """Sample blocks of an axis of n blocks: stride/2, stride/2 + stride, ..."""
    return (n + stride - 1 - stride // 2) // stride


def sample_strides(nx, ny):
    """The launcher's strides: kProbeStride per axis, halved while an axis has no sample, then the axis with more samples
    (x on a tie) doubled until at most kProbeMaxBlocks remain."""
    stx = sty = K_PROBE_STRIDE
    while stx > 1 and probe_samples(nx, stx) == 0:
        stx //= 2
    while sty > 1 and probe_samples(ny, sty) == 0:
        sty //= 2
    while probe_samples(nx, stx) * probe_samples(ny, sty) > K_PROBE_MAX_BLOCKS:
        if probe_samples(nx, stx) >= probe_samples(ny, sty):
            stx *= 2
        else:
            sty *= 2
    return stx, sty


def sample_blocks(nx, ny):
    """(bx, by) of the sample blocks in the probe's order (x fastest)."""
    stx, sty = sample_strides(nx, ny)
    sx, sy = probe_samples(nx, stx), probe_samples(ny, sty)
    return [(ix * stx + stx // 2, iy * sty + sty // 2) for iy in range(sy) for ix in range(sx)]


def row_sads(prev, cur, x0, bx, by, pred=(0, 0), delta=0):
    """SAD of every tile row against its row of every candidate window: [16 tile rows][17 dy][17 dx], candidate (dx, dy)
    at displacement (px + dx - 8, py + dy - 8); None when the block's windows leave the frame.

    The frames are looked at from the grid's moved origin org = x0 - 8 (1 on half-pixel grids), in a frame 2 org smaller;
    the tile of block (bx, by) starts at (16 bx + 8, 16 by + 8) there, its windows at (16 bx + px, 16 by + py);
    the newer frame is equalised, clamp(cur + delta)."""
    org = x0 - 8
    px, py = pred
    h, w = prev.shape
    H, Wb = h - 2 * org, w - 2 * org
    xf, yc0 = TILE * bx + px, TILE * by + py
    if xf < 0 or xf + 32 > Wb or yc0 < 0 or yc0 + 32 > H:
        return None
    ty, tx = org + TILE * by + 8, org + TILE * bx + 8
    tile = prev[ty:ty + TILE, tx:tx + TILE].astype(np.int64)
    win = np.clip(cur[org + yc0:org + yc0 + 32, org + xf:org + xf + 32].astype(np.int64) + delta, 0, 255)
    cand = sliding_window_view(win, (TILE, TILE))             # [dy][dx][row][col] = win[dy + row][dx + col]
    return np.abs(cand - tile).sum(axis=3).transpose(2, 0, 1)  # [row][dy][dx]


def bounds(rs, rows):
    """Per dy row: the smallest over its 17 dx of the SADs summed over `rows` of the tile -- a lower bound of every full
    SAD of that dy row."""
    return rs[list(rows)].sum(axis=0).min(axis=1)


def full_sad(rs, dy):
    """The best complete SAD of one dy row (what step B1 finds)."""
    return int(rs[:, dy, :].sum(axis=0).min())


def probe_word(prev, cur, x0, nx, ny, pred=(0, 0), delta=0):
    """The hint word of one pair at one level: verdict | separation << 8."""
    sads = [row_sads(prev, cur, x0, bx, by, pred, delta) for bx, by in sample_blocks(nx, ny)]
    survivors = survivors1 = rows = smallest2 = all2 = 0
    for rs in sads:
        if rs is None:
            continue
        two, one = bounds(rs, TWO_ROWS), bounds(rs, ONE_ROW)
        # a row could survive its bound when that is at most kFullOverBound (kFullOverOneRow) x the block's smallest one;
        # the block's own best row is evaluated completely either way and not counted
        survivors += int((two <= K_FULL_OVER_BOUND * two.min()).sum()) - 1
        survivors1 += int((one <= K_FULL_OVER_ONE_ROW * one.min()).sum()) - 1
        rows += K_SIDE - 1
        smallest2 += int(two.min())
        all2 += int(two.sum())
    # the best row's two-row bound against the mean of its block's, in per mille
    separation = smallest2 * K_SIDE * 1000 // all2 if all2 else 0
    verdict = 0 if rows and 100 * survivors > K_MAX_SURVIVORS_PCT * rows else 1
    if verdict == 1 and rows and 100 * survivors1 <= K_MAX_ONE_ROW_SURVIVORS_PCT * rows:
        verdict = 2
    if verdict == 0 and rows and separation <= K_MAX_SEPARATION_FOR_DEEPER_LOOK:
        # the deeper look, on every other sample block: the row with the first-smallest two-row bound evaluated completely,
        # and the rows whose four- or eight-row bound does not exceed that SAD counted
        surv4 = surv8 = n = 0
        for rs in sads[::2]:
            if rs is None:
                continue
            full = full_sad(rs, int(np.argmin(bounds(rs, TWO_ROWS))))
            surv4 += int((bounds(rs, FOUR_ROWS) <= full).sum()) - 1
            surv8 += int((bounds(rs, EIGHT_ROWS) <= full).sum()) - 1
            n += K_SIDE - 1
        if n and 100 * surv4 <= K_MAX_FOUR_ROW_SURVIVORS_PCT * n:
            verdict = 3
        elif n and 100 * surv8 <= K_MAX_EIGHT_ROW_SURVIVORS_PCT * n:
            verdict = 4
    return verdict | separation << 8


def frame_mean(img):
    """Round-half-up mean, as the equalisation takes it."""
    return (int(img.astype(np.int64).sum()) + img.size // 2) // img.size


def level0_word(p, prev, cur, pred=(0, 0)):
    """The word the probe of a level-0 search leaves for one pair of a context with params p (a dict or an object with
    the aof_params fields); pred: the level-1 predictor (the oracle's pred_x, pred_y)."""
    get = p.get if isinstance(p, dict) else (lambda k: getattr(p, k))
    assert get("tile") == TILE and get("search") == 8 and get("grid_mode") == 0
    x0 = 8 + (1 if get("subpixel") else 0)
    nx, ny = (get("width") - 2 * x0) // TILE, (get("height") - 2 * x0) // TILE
    delta = frame_mean(prev) - frame_mean(cur) if get("mean_subtract") else 0
    return probe_word(prev, cur, x0, nx, ny, pred, delta)
