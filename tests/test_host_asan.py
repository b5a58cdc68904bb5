"""ASan + UBSan over the product's host-only logic (parameter validation, grids, reduction chunks,
workspace layout, MAVLink packer), 20 000 random parameter sets including invalid ones; and over the rules the host
shares with the kernels (csrc/aof_mavlink.hpp, csrc/aof_exposure_step.hpp) compiled for the host: the kernels' packer
against the facade's, the two checksum steps on every input, the exposure bin and mean sample value; the column walk's
segment plan (csrc/aof_cols8_plan.hpp: cols_plan_make) on every case of tests/cols_plan_ref.py, field by field against
the Python model; the plans of the two coarse passes (csrc/aof_coarse_plan.hpp: coarse_plan_make, pyramid_plan_make) on
every case of tests/coarse_plan_ref.py and a list of extreme shapes, the same way; the plans of the small-pair kernels
(csrc/aof_small_plan.hpp: small_plan_make, lane8_group_plan) on every case of tests/small_plan_ref.py and its list of
extreme shapes, likewise; the plan of the flat lane-per-block launches (csrc/aof_lane8_plan.hpp: lane8_flat_plan) on every case of
tests/lane8_plan_ref.py, likewise, with xcd_remap (csrc/aof_xcd_remap.hpp, the text the kernels run) a permutation for every
total up to 4 096 and equal to the model's at every probe; the plan of a batch, the per-launch choice of a flat 8x8 launch
(csrc/aof_batch_plan.hpp: plan_batch, choose_lane8) and the launch plan of the 16x16 search (csrc/aof_tile16_plan.hpp: tile16_plan)
on every case of tests/batch_plan_ref.py, likewise; the launch plan of the warp kernel (csrc/aof_warp_plan.hpp: warp_plan_make) on
every case of tests/warp_plan_ref.py and its list of extreme shapes, likewise; fastdiv_make against the division it replaces; the stream bank's
bound per-stream tables (csrc/aof_bank_tables.hpp: what a binding call accepts, which tables a push uses and the order of its
refusals) and the flags of one per-stream table of OpticalFlowBank (facade/src/bank_table.hpp) over runs of ticks, both
against values written out in the selftest."""
import os
import subprocess

import batch_plan_ref as batch
import coarse_plan_ref as coarse
import cols_plan_ref as ref
import lane8_plan_ref as lane8
import small_plan_ref as small
import warp_plan_ref as warp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_logic_is_clean_under_asan_ubsan(tmp_path):
    pkg = os.path.join(ROOT, "aero-optical-flow_amd")
    exe = tmp_path / "host_selftest"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"),
           "-I" + os.path.join(pkg, "facade", "include"), "-I" + os.path.join(pkg, "facade", "src"),
           os.path.join(ROOT, "tests", "native", "host_selftest.cpp"), os.path.join(pkg, "csrc", "aof_params.cpp"),
           os.path.join(pkg, "facade", "src", "optical_flow_rad.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, timeout=300)
    cases = ref.CPU_CASES + ref.GPU_CASES + ref.PLAN_ONLY
    listing = tmp_path / "cols_plan_cases.txt"
    listing.write_text("".join(ref.selftest_line(c) + "\n" for c in cases))
    coarse_cases = coarse.CPU_CASES + coarse.GPU_CASES + coarse.PLAN_ONLY
    lines = [coarse.selftest_lines(c) for c in coarse_cases]
    coarse_listing, pyramid_listing = tmp_path / "coarse_plan_cases.txt", tmp_path / "pyramid_plan_cases.txt"
    coarse_listing.write_text("".join(a + "\n" for a, _ in lines))
    pyramid_listing.write_text("".join(b + "\n" for _, b in lines))
    small_cases = small.CPU_CASES + small.GPU_CASES + small.PLAN_ONLY
    small_listing = tmp_path / "small_plan_cases.txt"
    small_listing.write_text("".join(small.selftest_line(c) + "\n" for c in small_cases))
    lane8_listing, xcd_listing = tmp_path / "lane8_plan_cases.txt", tmp_path / "xcd_probes.txt"
    lane8_listing.write_text("".join(lane8.selftest_line(c) + "\n" for c in lane8.CASES))
    xcd_probes = lane8.xcd_probes()
    xcd_listing.write_text("".join(f"{total} {b}\n" for total, b in xcd_probes))
    batch_cases, tile16_cases, choose_rows = batch.batch_cases(), batch.tile16_cases(), batch.choose_rows()
    batch_listing, tile16_listing, choose_listing = tmp_path / "batch_plan_cases.txt", tmp_path / "tile16_plan_cases.txt", tmp_path / "choose_lane8_rows.txt"
    batch_listing.write_text("".join(batch.selftest_line(c) + "\n" for c in batch_cases))
    tile16_listing.write_text("".join(batch.tile16_line(c) + "\n" for c in tile16_cases))
    choose_listing.write_text("".join(batch.choose_line(r) + "\n" for r in choose_rows))
    warp_cases = warp.WARP_CASES + warp.WARP_PLAN_ONLY
    warp_listing = tmp_path / "warp_plan_cases.txt"
    warp_listing.write_text("".join(warp.warp_selftest_line(c) + "\n" for c in warp_cases))
    r = subprocess.run([str(exe), str(listing), str(coarse_listing), str(pyramid_listing), str(small_listing), str(lane8_listing),
                        str(xcd_listing), str(batch_listing), str(tile16_listing), str(choose_listing), str(warp_listing)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout}{r.stderr}"
    assert "valid parameter sets" in r.stdout
    assert "packer: 4012 frames equal to the facade's, lengths 52 and 56" in r.stdout
    assert "checksum: both steps and the facade's agree on 65536 x 256 inputs" in r.stdout
    assert "exposure: 256 bins and 2002 mean sample values equal to the public functions" in r.stdout
    # the bank's bound tables and the facade's table flags: every case equal to the value written in the selftest
    tables = [int(line.split()[4]) for line in r.stdout.splitlines() if line.startswith("host selftest: bank tables: ")]
    assert len(tables) == 1 and tables[0] >= 25, r.stdout
    assert "host selftest: facade table: 21 steps, copies and bindings as written" in r.stdout
    assert "fast_div: 20416 divisors, all numerators below 65536 and up to 196 around multiples up to 2^31 equal to n / d" in r.stdout
    # cols_plan_make == the model, on every case of every list
    assert f"cols plan: {len(cases)} cases" in r.stdout and len(cases) >= 60
    plans = [line.split()[2:] for line in r.stdout.splitlines() if line.startswith("cols plan: ")]
    assert len(plans) == len(cases)
    for c, got in zip(cases, plans):
        want = ref.plan_fields(ref.plan_of(c))
        assert len(got) == len(want) == len(ref.PLAN_FIELDS)
        diff = {name: (int(g), w) for name, g, w in zip(ref.PLAN_FIELDS, got, want) if int(g) != w}
        assert not diff, (c["id"], diff)
    # coarse_plan_make and pyramid_plan_make == the model, on every case of every list
    assert f"coarse plan: {len(coarse_cases)} cases" in r.stdout and f"pyramid plan: {len(coarse_cases)} cases" in r.stdout
    assert len(coarse_cases) >= 90 and len(coarse.PLAN_ONLY) >= 20
    for tag, fields, names, which in (("coarse plan: ", coarse.coarse_fields, coarse.COARSE_FIELDS, 0),
                                      ("pyramid plan: ", coarse.pyramid_fields, coarse.PYRAMID_FIELDS, 1)):
        plans = [line.split()[2:] for line in r.stdout.splitlines() if line.startswith(tag)]
        assert len(plans) == len(coarse_cases)
        for c, got in zip(coarse_cases, plans):
            want = fields(coarse.plans_of(c)[which])
            assert len(got) == len(want) == len(names)
            diff = {name: (int(g), w) for name, g, w in zip(names, got, want) if int(g) != w}
            assert not diff, (tag, c["id"], diff)
    verdicts = {coarse.plans_of(c)[0]["verdict"] for c in coarse_cases}
    assert verdicts == set(coarse.VERDICTS), set(coarse.VERDICTS) - verdicts
    # small_plan_make and lane8_group_plan == the model, on every case of every list
    assert f"small plan: {len(small_cases)} cases" in r.stdout and len(small_cases) >= 70 and len(small.PLAN_ONLY) >= 30
    for tag, fields, names, which in (("small plan: ", small.plan_fields, small.PLAN_FIELDS, 0), ("group plan: ", small.group_fields, small.GROUP_FIELDS, 1)):
        plans = [line.split()[2:] for line in r.stdout.splitlines() if line.startswith(tag)]
        assert len(plans) == len(small_cases)
        for c, got in zip(small_cases, plans):
            want = fields(small.plans_of(c)[which])
            assert len(got) == len(want) == len(names)
            diff = {name: (int(g), w) for name, g, w in zip(names, got, want) if int(g) != w}
            assert not diff, (tag, c["id"], diff)
    # every verdict occurs, and the grouped plan both applies and does not
    assert {small.plans_of(c)[0]["verdict"] for c in small_cases} == set(small.VERDICTS)
    assert {small.plans_of(c)[1]["ppw"] > 0 for c in small_cases} == {True, False}
    # lane8_flat_plan == the model, on every case of every list; xcd_remap == the model's at every probe
    assert f"lane8 plan: {len(lane8.CASES)} cases" in r.stdout and len(lane8.CASES) >= 85 and len(lane8.PLAN_ONLY) >= 35
    plans = [line.split()[2:] for line in r.stdout.splitlines() if line.startswith("lane8 plan: ")]
    assert len(plans) == len(lane8.CASES)
    for c, got in zip(lane8.CASES, plans):
        want = lane8.plan_fields(lane8.plan_of(c))
        assert len(got) == len(want) == len(lane8.PLAN_FIELDS)
        diff = {name: (int(g), w) for name, g, w in zip(lane8.PLAN_FIELDS, got, want) if int(g) != w}
        assert not diff, (c["id"], diff)
    assert f"xcd_remap: a permutation for every total up to 4096, {len(xcd_probes)} probes" in r.stdout and len(xcd_probes) >= 1000
    remapped = [int(line.split()[2]) for line in r.stdout.splitlines() if line.startswith("xcd remap: ")]
    assert remapped == [int(lane8.xcd_remap(b, total)) for total, b in xcd_probes]
    # plan_batch, tile16_plan and choose_lane8 == the model, on every case of every list; every kind and verdict occurs
    assert f"batch plan: {len(batch_cases)} cases" in r.stdout and len(batch_cases) >= 250
    assert f"tile16 plan: {len(tile16_cases)} cases" in r.stdout and len(tile16_cases) >= 30
    assert f"{len(choose_rows)} rows printed" in r.stdout and len(choose_rows) >= 1000
    for tag, cases, fields, names in (("batch plan: ", batch_cases, lambda c: batch.plan_fields(batch.plan(c)), batch.PLAN_FIELDS),
                                      ("tile16 plan: ", tile16_cases, lambda c: batch.tile16_fields(batch.tile16_plan(c)), batch.T16_FIELDS),
                                      ("choose lane8: ", choose_rows, batch.choose_row, batch.CHOOSE_FIELDS)):
        plans = [line.split()[2:] for line in r.stdout.splitlines() if line.startswith(tag)]
        assert len(plans) == len(cases)
        for c, got in zip(cases, plans):
            want = fields(c)
            assert len(got) == len(want) == len(names)
            diff = {name: (int(g), w) for name, g, w in zip(names, got, want) if int(g) != w}
            assert not diff, (tag, c["id"], diff)
    planned = [batch.plan(c) for c in batch_cases]
    assert {k for pl in planned for k in pl["kind"] if k} == set(batch.SEARCH_KINDS)
    assert {pl["coarse"] for pl in planned} == set(batch.COARSE_KINDS)
    assert {pl["small"] for pl in planned} == {True, False} and {pl["valid"] for pl in planned} == {True, False}
    assert any(pl["small_class"] and not pl["small"] for pl in planned) and any(pl["sequence"] and not pl["k1_pass"] for pl in planned)
    assert any(pl["kind"][0] == "tile16" and pl["prune"][0] == 0 and c["mode"] != 0 for c, pl in zip(batch_cases, planned)), "search_kind clears prune"
    assert {batch.tile16_plan(c)["verdict"] for c in tile16_cases} == set(batch.T16_VERDICTS)
    assert {batch.tile16_plan(c)["front"] for c in tile16_cases} == set(batch.FRONTS)
    assert {(pl["overflow"], pl["refused"]) for pl in map(batch.tile16_plan, tile16_cases)} == {(0, 0), (0, 1), (1, 1)}
    chosen = [batch.choose_row(r) for r in choose_rows]
    assert {(row[0], row[1], row[2]) for row in chosen} >= {(0, 0, 0), (0, 0, 1), (1, 1, 1), (2, 1, 0), (1, 0, 0), (2, 0, 0)}
    census = [line for line in r.stdout.splitlines() if line.startswith("host selftest: batch plan:") or line.startswith("host selftest: tile16 plan:")]
    assert len(census) == 2 and all(int(v) > 0 for line in census for v in line.replace(",", "").split()[6:] if v.isdigit()), census
    assert "host selftest: choose lane8: 17 rows equal to the values written" in r.stdout
    # warp_plan_make == the model, on every case of both lists; every verdict occurs
    assert f"warp plan: {len(warp_cases)} cases" in r.stdout and len(warp_cases) >= 30 and len(warp.WARP_PLAN_ONLY) >= 20
    plans = [line.split()[2:] for line in r.stdout.splitlines() if line.startswith("warp plan: ")]
    assert len(plans) == len(warp_cases)
    for c, got in zip(warp_cases, plans):
        want = warp.warp_fields(warp.warp_plan(**warp.warp_plan_args(c)))
        assert len(got) == len(want) == len(warp.WARP_FIELDS)
        diff = {name: (int(g), w) for name, g, w in zip(warp.WARP_FIELDS, got, want) if int(g) != w}
        assert not diff, (c["id"], diff)
    assert {warp.warp_plan(**warp.warp_plan_args(c))["verdict"] for c in warp_cases} == set(warp.VERDICTS)
    assert {(pl["vec"], pl["attr"], pl["zero_hist"]) for pl in (warp.warp_plan(**warp.warp_plan_args(c)) for c in warp_cases)} >= {
        (1, 0, 0), (0, 0, 0), (1, 1, 0), (1, 0, 1), (0, 0, 1), (0, 1, 0)}
