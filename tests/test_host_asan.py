"""ASan + UBSan over the product's host-only logic and the rules the host shares with the kernels, compiled for the host into
one stand-alone program (tests/native/host_selftest.cpp) that is built once and run once per named check.  A check without a
case file holds values written in the program and is held here to its summary sentence.  A plan family is a check with a case
file: the model lists its cases, the program prints the C++ function's plan of each, and the test compares field by field under
the model's names.  What a family holds is said where its model defines it (selftest_families):

  family                                  C++ function (csrc/)                                      model (tests/)
  cols-plan                               aof_cols8_plan.hpp: cols_plan_make                        cols_plan_ref.py
  coarse-plan, pyramid-plan               aof_coarse_plan.hpp: coarse_plan_make, pyramid_plan_make  coarse_plan_ref.py
  small-plan, group-plan (one listing)    aof_small_plan.hpp: small_plan_make, lane8_group_plan     small_plan_ref.py
  lane8-plan, xcd-probes                  aof_lane8_plan.hpp: lane8_flat_plan; aof_xcd_remap.hpp    lane8_plan_ref.py
  batch-plan, tile16-plan, choose-lane8   aof_batch_plan.hpp, aof_tile16_plan.hpp                   batch_plan_ref.py
  warp-plan                               aof_warp_plan.hpp: warp_plan_make                         warp_plan_ref.py

The compiler is $CXX (default c++), as for the other sanitized programs; this file used to name g++."""
import functools

import pytest

import batch_plan_ref as batch
import coarse_plan_ref as coarse
import cols_plan_ref as ref
import lane8_plan_ref as lane8
import selftest_rig as rig
import small_plan_ref as small
import warp_plan_ref as warp

PKG = "aero-optical-flow_amd/"
FAMILIES = [f for model in (ref, coarse, small, lane8, batch, warp) for f in model.selftest_families()]
CASES = {f.name: f.cases for f in FAMILIES}


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    """run(check): the completed `host_selftest <check> [listing]`, the listing written from the check's family; each check
    runs once however many tests read its output."""
    out = tmp_path_factory.mktemp("host_selftest")
    exe = rig.build(out, "host_selftest", ["tests/native/host_selftest.cpp", PKG + "csrc/aof_params.cpp", PKG + "facade/src/optical_flow_rad.cpp"],
                    extra_includes=(PKG + "facade/include", PKG + "facade/src"))

    @functools.lru_cache(maxsize=None)
    def run(check):
        fam = next((f for f in FAMILIES if f.check == check), None)
        listing = out / (check + ".txt")
        if fam:
            listing.write_text("".join(fam.line(c) + "\n" for c in fam.cases))
        r = rig.run(exe, check, *([str(listing)] if fam else []))
        assert r.returncode == 0, f"rc={r.returncode}\n{r.stdout[-2000:]}{r.stderr}"
        return r.stdout

    return run


# ---- the checks that hold values written in the program ----------------------------------------------------------------------

def test_host_logic_is_clean_under_asan_ubsan(selftest):
    """Parameter validation, grids, reduction chunks, workspace layout on 20 000 random parameter sets including invalid ones;
    the facade's packer on random messages."""
    assert "valid parameter sets" in selftest("params")
    assert "host selftest: packer range: 2000 frames" in selftest("packer-range")


# The kernels' packer against the facade's, the two checksum steps on every input, the shared exposure bin and mean sample value
# against the public functions, fastdiv_make against the division it replaces, the flags of one per-stream table of
# OpticalFlowBank (facade/src/bank_table.hpp) over runs of ticks, choose_lane8 row by row, xcd_remap (the text the kernels run).
WRITTEN = {
    "packer": "packer: 4012 frames equal to the facade's, lengths 52 and 56",
    "checksum": "checksum: both steps and the facade's agree on 65536 x 256 inputs",
    "exposure": "exposure: 256 bins and 2002 mean sample values equal to the public functions",
    "fastdiv": "fast_div: 20416 divisors, all numerators below 65536 and up to 196 around multiples up to 2^31 equal to n / d",
    "facade-table": "host selftest: facade table: 21 steps, copies and bindings as written",
    "choose-lane8-written": "host selftest: choose lane8: 17 rows equal to the values written",
    "xcd-permutation": "xcd_remap: a permutation for every total up to 4096",
}


@pytest.mark.parametrize("check", WRITTEN)
def test_the_check_holds_the_values_written_in_it(selftest, check):
    assert WRITTEN[check] in selftest(check)


def test_the_banks_bound_tables_equal_the_values_written(selftest):
    """What a binding call accepts, which tables a push uses and the order of its refusals (csrc/aof_bank_tables.hpp)."""
    stdout = selftest("bank-tables")
    tables = [int(line.split()[4]) for line in stdout.splitlines() if line.startswith("host selftest: bank tables: ")]
    assert len(tables) == 1 and tables[0] >= 25, stdout


# ---- the plan families -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES, ids=lambda f: f.name)
def test_the_plan_equals_its_model_on_every_case(selftest, fam):
    stdout = selftest(fam.check)
    assert fam.summary.format(len(fam.cases)) in stdout
    plans = [line.split()[2:] for line in stdout.splitlines() if line.startswith(fam.tag)]
    assert len(plans) == len(fam.cases)
    for c, got in zip(fam.cases, plans):
        want = fam.want(c)
        assert len(got) == len(want) == len(fam.names)
        diff = {name: (int(g), w) for name, g, w in zip(fam.names, got, want) if int(g) != w}
        assert not diff, (fam.tag, c["id"], diff)


# ---- the censuses: the lists are long enough, and every verdict and kind occurs among their cases --------------------------------

def test_cols_census():
    assert len(CASES["cols-plan"]) >= 60


def test_coarse_census():
    cases = CASES["coarse-plan"]
    assert CASES["pyramid-plan"] is cases
    assert len(cases) >= 90 and len(coarse.PLAN_ONLY) >= 20
    verdicts = {coarse.plans_of(c)[0]["verdict"] for c in cases}
    assert verdicts == set(coarse.VERDICTS), set(coarse.VERDICTS) - verdicts


def test_small_census():
    """Every verdict occurs, and the grouped plan both applies and does not."""
    cases = CASES["small-plan"]
    assert CASES["group-plan"] is cases
    assert len(cases) >= 70 and len(small.PLAN_ONLY) >= 30
    assert {small.plans_of(c)[0]["verdict"] for c in cases} == set(small.VERDICTS)
    assert {small.plans_of(c)[1]["ppw"] > 0 for c in cases} == {True, False}


def test_lane8_census():
    assert CASES["lane8-plan"] is lane8.CASES
    assert len(lane8.CASES) >= 85 and len(lane8.PLAN_ONLY) >= 35
    assert len(CASES["xcd-probes"]) >= 1000


def test_batch_census(selftest):
    """Every kind and verdict occurs, in the model and in the program's own count."""
    batch_cases, tile16_cases, choose_rows = CASES["batch-plan"], CASES["tile16-plan"], CASES["choose-lane8"]
    assert len(batch_cases) >= 250
    assert len(tile16_cases) >= 30
    assert len(choose_rows) >= 1000
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
    stdout = selftest("batch-plan") + selftest("tile16-plan")
    census = [line for line in stdout.splitlines() if line.startswith("host selftest: batch plan:") or line.startswith("host selftest: tile16 plan:")]
    assert len(census) == 2 and all(int(v) > 0 for line in census for v in line.replace(",", "").split()[6:] if v.isdigit()), census


def test_warp_census():
    """Every verdict occurs."""
    cases = CASES["warp-plan"]
    assert len(cases) >= 30 and len(warp.WARP_PLAN_ONLY) >= 20
    planned = [warp.selftest_plan(c) for c in cases]
    assert {pl["verdict"] for pl in planned} == set(warp.VERDICTS)
    assert {(pl["vec"], pl["attr"], pl["zero_hist"]) for pl in planned} >= {(1, 0, 0), (0, 0, 0), (1, 1, 0), (1, 0, 1), (0, 0, 1), (0, 1, 0)}
