"""What the device tests of the 16x16 search share: the hard-inputs batch, the frames of the block-row cases
(tests/tile16_rows_ref.py), the frame arena with its guard zones, one batch run on junk-filled outputs and workspace, the
oracle's records of a batch, and the byte-for-byte comparison of the two (tests/test_gpu_tile16_verdicts.py,
tests/test_gpu_tile16_plan.py, tests/test_gpu_tile16_rows.py)."""
import numpy as np

PATTERN = 0x5A5A00                      # what the fill kernel writes above the verdict (the probe's separation figure)
JUNK = 0xA7                             # workspace and output bytes on entry
GUARD, FRAME_SENTINEL = 4096, 0x5C      # the zones around the frames of a FrameArena


def hard_batch(synth, W, H, two_level):
    """(prevs, curs, names): translations, sensor noise, unrelated / identical / flat / half-flat frames, ties on periodic
    textures, a checkerboard against its inverse, a saturating brightness step; two-level batches add a horizontal-only
    motion (the predictor's column shift and tail guard) and one near the +-17 reach (windows pushed out of the frame)."""
    reach = 17 if two_level else 8
    pairs = []
    for k, noise in enumerate((0, 0, 3, 8, 16, 40)):
        p, c, _ = synth.make_pair(W, H, reach, 4100 + k, noise=noise)
        pairs.append((f"noise{noise}" if noise else f"clean{k}", p, c))
    rng = np.random.default_rng(41)
    tex = synth.make_pair(W, H, reach, 4110)[0]
    pairs.append(("unrelated", tex, rng.integers(0, 256, (H, W), dtype=np.uint8)))
    pairs.append(("identical", tex, tex.copy()))
    flat = np.full((H, W), 90, np.uint8)
    pairs.append(("flat", flat, flat.copy()))
    half = rng.integers(0, 256, (H, W), dtype=np.uint8)
    half[:, : W // 2] = 90
    pairs.append(("half_flat", half, half.copy()))
    px2 = np.zeros((H, W), np.uint8); px2[:, 0::2] = 200
    py2 = np.zeros((H, W), np.uint8); py2[0::2, :] = 150
    dots = np.zeros((H, W), np.uint8); dots[0::4, 0::4] = 255
    pairs += [("period2_x", px2, px2.copy()), ("period2_y", py2, py2.copy()), ("dots", dots, dots.copy())]
    yy, xx = np.mgrid[0:H, 0:W]
    chk = (((xx // 16 + yy // 16) % 2) * 255).astype(np.uint8)
    pairs.append(("checker_inverse", chk, 255 - chk))
    p, c, _ = synth.make_pair(W, H, reach, 4120, shift=(3, -2), brightness=120)
    pairs.append(("bright_step", p, c))
    if two_level:
        p, c, _ = synth.make_pair(W, H, reach, 4130, shift=(13, 0))
        pairs.append(("horizontal", p, c))
        p, c, _ = synth.make_pair(W, H, reach, 4140, shift=(-16, 17))
        pairs.append(("reach", p, c))
    return np.stack([q[1] for q in pairs]), np.stack([q[2] for q in pairs]), [q[0] for q in pairs]


# ---- the block-row cases ------------------------------------------------------------------------------------------------

def case_params(aof, c):
    kw = dict(tile=16, search=8, value_threshold=12000, min_valid=0)
    if c["sub"]:
        kw["subpixel"] = 1
    if c["levels"] == 2:
        kw["pyramid_levels"] = 2
    if c["eq"]:
        kw["mean_subtract"] = 1
    if c.get("gate_off"):
        kw["feature_threshold"] = 0     # (flat tiles are searched too)
    return aof.default_params(c["w"], c["h"], **kw)


def case_frames(c, synth, rows_ref, k=0):
    """(prevs, curs, names) of batch k of a case of tile16_rows_ref.CASES."""
    W, H = c["w"], c["h"]
    reach = 17 if c["levels"] == 2 else 8
    mk = lambda seed, **kw: synth.make_pair(W, H, reach, seed, **kw)[:2]
    if c["frames"] == "designed":
        # a clean translation, a frame against unrelated noise, the corner of the reach under +-8 LSB, a noisy translation
        out, names = [], []
        for i in range(c["n_pairs"]):
            kind = ("clean", "unrelated", "reach", "noise8")[i % 4]
            seed = 5300 + 16 * i + c["nx"]
            if kind == "unrelated":
                pair = (mk(seed)[0], np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8))
            else:
                pair = mk(seed, **dict(clean=dict(shift=(5, -3)), reach=dict(shift=(-8, 8), noise=8), noise8=dict(shift=(-2, 6), noise=8))[kind])
            out.append(pair); names.append(f"{kind}{i}")
    elif c["frames"] in ("h-shifts", "v-shifts"):
        shifts = rows_ref.H_SHIFTS if c["frames"] == "h-shifts" else rows_ref.V_SHIFTS
        out = [mk(5400 + i, shift=s) for i, s in enumerate(shifts)]
        names = [f"shift{s}" for s in shifts]
    elif c["frames"] == "ring":
        # texture k at the reach, last of its batch: the bottom-right (8, 8) or bottom-left (-8, 8) block's ring lies on the
        # frame's last row; a brightness step, so that an equalised context has a delta
        n = rows_ref.batch_pairs(c, k)
        last = (8, 8) if k % 2 == 0 else (-8, 8)
        out = [mk(5500 + 7 * k + q, noise=k % 3, brightness=5 + 4 * (k % 4), **(dict(shift=last) if q == n - 1 else {})) for q in range(n)]
        names = [f"texture{k}-{q}" for q in range(n)]
    elif c["frames"] == "bright-steps":
        # the hard-inputs batch's step (+120: cur saturates at 255) at three displaced shifts, and a contrast stretch with a
        # step, whose cur clamps at both ends and whose dark pixels the staging's negative delta clamps at 0
        shifts = [(13, 0), (-5, 2), (3, -2)]
        out = [mk(5600 + i, shift=s, brightness=120) for i, s in enumerate(shifts)] + [mk(5603, shift=(-7, 1), brightness=60, contrast=2.5)]
        names = [f"bright{s}" for s in shifts] + ["stretched(-7, 1)"]
    elif c["frames"] == "corners":
        out, names = corner_pairs(c, k, rows_ref.batch_pairs(c, k))
    else:
        raise KeyError(c["frames"])
    return np.stack([q[0] for q in out]), np.stack([q[1] for q in out]), names


CORNER_DIRS = {1: (8, 8), 5: (-8, -8)}      # direction won (down-right, up-left) and the match it is built at


def corner_blocks(c):
    """(by, bx, direction) of the two designed blocks of a "corners" pair: the bottom-right block, whose ring's last byte
    at (8, 8) is the last of row 32's bytewise copy on the frame's last row, and the top-left block, whose ring's first
    byte at (-8, -8) is the pad byte in front of row -1 (the frame's first byte)."""
    return [(c["ny"] - 1, c["nx"] - 1, 1), (0, 0, 5)]


def corner_pairs(c, k, n):
    """Unrelated noise frames; in the LAST pair two blocks are built so that ONE ring byte decides the half-pixel
    direction.  The tile is flat v but for one corner pixel v + 1; cur is flat v where the direction's averages read
    (the matched tile, and the ring's row and column on the direction's side) but for the ring's corner byte, v + 4: the
    diagonal average there is havg(v, havg(v, v + 4)) = v + 1, the direction's SAD 0 against the match's SAD 1.  Any
    other value of that byte but v + 4 .. v + 7 leaves the direction at the match's SAD or above: no direction wins.  The
    ring's other row and column are far off v, so that no neighbouring candidate ties with the match."""
    W, H, v = c["w"], c["h"], 60 + 30 * k
    rng = np.random.default_rng(5700 + k)
    out = [(rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)) for _ in range(n)]
    prev, cur = out[-1]
    for by, bx, d in corner_blocks(c):
        (dx, dy), x, y = CORNER_DIRS[d], 9 + 16 * bx, 9 + 16 * by
        prev[y:y + 16, x:x + 16] = v
        mx, my = x + dx, y + dy
        cur[my - 1:my + 17, mx - 1:mx + 17] = v + 50
        if d == 1:
            cur[my:my + 17, mx:mx + 17] = v
            prev[y + 15, x + 15], cur[my + 16, mx + 16] = v + 1, v + 4
            assert (my + 16, mx + 16) == (H - 1, W - 15)
        else:
            cur[my - 1:my + 16, mx - 1:mx + 16] = v
            prev[y, x], cur[my - 1, mx - 1] = v + 1, v + 4
            assert (my - 1, mx - 1) == (0, 0)
    return out, [f"corners{k}-{q}" for q in range(n)]


def assert_predictor_census(c, preds, prevs, curs, rows_ref):
    """What a two-level case is in the list for, from the oracle's predictors (the flow records' pred_x, pred_y)."""
    groups = [[rows_ref.workgroup(c["w"], c["h"], c["org"], c["nx"], c["ny"], by, px, py, i, len(preds), c["w"] * c["h"], 0, bool(c["sub"]))
               for by in range(c["ny"])] for i, (px, py) in enumerate(preds)]
    if c["frames"] == "h-shifts":
        assert {px & 15 for px, _ in preds} == set(range(16)), c["id"]
        assert {px >> 4 for px, _ in preds} == ({-2, -1, 0, 1} if c["sub"] else {-1, 0, 1}), (c["id"], sorted({px >> 4 for px, _ in preds}))
        assert any(g["rows_ok"] and g["skip_left"] for gs in groups for g in gs) and any(g["rows_ok"] and g["skip_right"] for gs in groups for g in gs)
        if not c["sub"]:
            # H % 16 == 0: the bottom block row of every pair with a displaced copy ends on the frame's last byte, unless the
            # predictor moves the row as well (up: the copy ends inside the frame; down: the block row is skipped)
            assert c["h"] % 16 == 0
            taken = [gs[-1]["tail_guard"] for gs in groups]
            assert taken == [bool(px & 15) and py == 0 for px, py in preds] and sum(taken) >= 4, list(zip(preds, taken))
    elif c["frames"] == "v-shifts":
        out = {(gs[0]["rows_ok"], all(g["rows_ok"] for g in gs[1:-1]), gs[-1]["rows_ok"]) for gs in groups}
        assert {(False, True, True), (True, True, False)} <= out, (c["id"], preds, out)       # the top row only, the bottom row only
    elif c["frames"] == "bright-steps":
        assert all(px & 15 for px, _ in preds), preds
        # every cur saturates at 255 under its step; the staging's delta (about minus the step) clamps dark pixels at 0 somewhere
        steps = [float(cur.astype(int).mean() - prev.astype(int).mean()) for prev, cur in zip(prevs, curs)]
        assert all((cur == 255).any() for cur in curs) and min(steps) > 30, steps
        assert any((cur < step - 2).any() for cur, step in zip(curs, steps)), "no pixel that the delta clamps at 0"
    else:
        raise KeyError(c["frames"])


def preds_of(refs):
    return [(int(r["flow"]["pred_x"]), int(r["flow"]["pred_y"])) for r in refs]


BOUND_ROWS = {1: (4, 12), 2: (4,), 3: (2, 6, 10, 14), 4: tuple(range(0, 16, 2))}   # tile rows of step A's bound by verdict


def b2_list_sizes(prev, cur, nx, ny, hint):
    """One level, no half-pixel: per block row, the entries of step B2's list (the items whose step-A bound does not exceed
    their block's best SAD after step B1), and the blocks' smallest complete SADs -- numpy sums of the oracle's SAD."""
    from numpy.lib.stride_tricks import sliding_window_view
    sizes, best = [], np.zeros((ny, nx), np.int64)
    for by in range(ny):
        listed = 0
        for bx in range(nx):
            ref = prev[16 * by + 8:16 * by + 24, 16 * bx + 8:16 * bx + 24].astype(np.int64)
            win = sliding_window_view(cur[16 * by:16 * by + 32, 16 * bx:16 * bx + 32].astype(np.int64), (16, 16))   # [dy, dx, r, c]
            rows = np.abs(win - ref).sum(axis=3)                                                                     # [dy, dx, r]
            full = rows.sum(axis=2)
            bound = rows[:, :, list(BOUND_ROWS[hint])].sum(axis=2).min(axis=1)                                       # [dy]
            b1 = int(np.argmin(bound))            # (the first smallest bound)
            after_b1 = int(full[b1].min())
            listed += int(sum(1 for d in range(17) if d != b1 and bound[d] <= after_b1))
            best[by, bx] = full.min()
        sizes.append(listed)
    return sizes, best


class FrameArena:
    """prev and cur frames of a batch in one allocation, a guard zone in front, between and behind (the last pair's last
    byte lies against it); tp, tc are the views a launch gets."""

    def __init__(self, torch, device, prevs, curs):
        n, h, w = prevs.shape
        size = n * h * w
        assert size % 16 == 0
        self.mem = torch.full((3 * GUARD + 2 * size,), FRAME_SENTINEL, dtype=torch.uint8, device=device)
        self.tp = self.mem[GUARD:GUARD + size].view(n, h, w)
        self.tc = self.mem[2 * GUARD + size:2 * GUARD + 2 * size].view(n, h, w)
        self.tp.copy_(torch.from_numpy(prevs.copy())); self.tc.copy_(torch.from_numpy(curs.copy()))   # (the cached frames are read-only)
        assert self.tp.data_ptr() % 16 == 0 and self.tc.data_ptr() % 16 == 0
        self.held = self.mem.cpu().numpy().copy()
        g = self.held
        assert (g[:GUARD] == FRAME_SENTINEL).all() and (g[-GUARD:] == FRAME_SENTINEL).all() and (g[GUARD + size:2 * GUARD + size] == FRAME_SENTINEL).all()

    def assert_untouched(self, what):
        now = self.mem.cpu().numpy()
        bad = np.flatnonzero(now != self.held)
        assert bad.size == 0, (what, "frames or their guards written", bad[:8])


# ---- one launch -----------------------------------------------------------------------------------------------------------

def oracle_refs(orc, p, prevs, curs):
    po = orc.params_from(p)
    return [orc.flow_pair(po, prevs[i], curs[i], want_l1=True) for i in range(prevs.shape[0])]


def run(aof, eng, p, tp, tc, device, verdicts=None):
    """One batch on junk-filled outputs and workspace; verdicts None: whatever the context is set to."""
    import torch
    n = tp.shape[0]
    L = aof.workspace_layout(p, n)
    nb0, nb1 = eng.nblocks(0), eng.nblocks(1) if p.pyramid_levels == 2 else 0
    ws = torch.full((L.total_bytes,), JUNK, dtype=torch.uint8, device=device)
    blocks = torch.full((n, nb0), JUNK * 0x01010101 - (1 << 32), dtype=torch.int32, device=device)
    flows = torch.full((n, 16), JUNK, dtype=torch.uint8, device=device)
    subdirs = torch.full((n, nb0), JUNK, dtype=torch.uint8, device=device) if p.subpixel else None
    if verdicts is not None:
        eng.debug_tile16_verdicts(verdicts)
    eng.flow_batch(tp, tc, blocks=blocks, subdirs=subdirs, flows=flows, workspace=ws)
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    return dict(blocks=aof.blocks_view(blocks), flows=aof.flows_view(flows),
                subdirs=subdirs.cpu().numpy() if subdirs is not None else None,
                l1=w[L.l1_blocks:L.l1_blocks + 4 * n * nb1].view(aof.BLOCK_DTYPE).reshape(n, nb1) if nb1 else None,
                hints=w[L.hints:L.hints + 4 * n].view(np.uint32).copy())


def assert_matches(got, refs, names, what, l1=False, exhaustive=None):
    for i, r in enumerate(refs):
        key = (what, i, names[i])
        assert got["blocks"][i].tobytes() == r["blocks"].tobytes(), key
        assert got["flows"][i].tobytes() == r["flow"].tobytes(), key
        if got["subdirs"] is not None:
            assert got["subdirs"][i].tobytes() == r["subdirs"].tobytes(), key
        if l1:
            assert got["l1"][i].tobytes() == r["blocks_l1"].tobytes(), key
    if exhaustive is not None:
        for k in ("blocks", "flows", "subdirs", "l1"):
            if got[k] is not None:
                assert got[k].tobytes() == exhaustive[k].tobytes(), (what, k)
