"""What the device tests of the 16x16 search share: one batch run on junk-filled outputs and workspace, the oracle's records
of a batch, and the byte-for-byte comparison of the two (tests/test_gpu_tile16_verdicts.py, tests/test_gpu_tile16_plan.py)."""
import numpy as np

PATTERN = 0x5A5A00                      # what the fill kernel writes above the verdict (the probe's separation figure)
JUNK = 0xA7                             # workspace and output bytes on entry


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
