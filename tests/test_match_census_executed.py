"""The executed model of tools/match_isa_census.py (no GPU: hipcc -S once, the rest on recorded figures).

The static census counts every loop body outside the scan once and leaves lane 0's tail out; the executed model gives the
loops their trips as a function of Kf, splits the tail by path and adds a launch up from its survivors, non-survivors and
void slots (docs/match_tail.md).  Checked here:
  * on the figures recorded from the PARENT of that change (tests/golden/match_census_parent_figures.json, the tool's own
    --json output on the parent's assembly) the benchmark's launch -- 2 000 survivors, 8 000 non-survivors, 1 506 void slots
    at K = 500 -- comes out within 5 % of the 75.90 M that SQ_INSTS_VALU counted for that build (docs/match_repair_once.md),
    vector and matrix instructions together, which is what that counter holds;
  * on the current source, for mixes given on the command line, the tool reproduces its own tables: the same figures fed
    back through --figures give the same launches, each launch is the sum of its parts, and the parts follow the trip
    counts of the per-loop figures."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "match_isa_census.py")
PARENT = os.path.join(ROOT, "tests", "golden", "match_census_parent_figures.json")
COUNTED_PARENT = 75.90e6          # SQ_INSTS_VALU of k_match_split per launch, counters-only run, at the parent
MIXES = ["500,500,2000,8000,1506", "257,500,10,20,3", "1000,1000,100,400,12", "20,500,0,5,0"]


def _tool(*args):
    r = subprocess.run([sys.executable, TOOL, "--json"] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


def test_parent_launch_total_against_the_counter():
    r = _tool("--figures", PARENT)
    L = r["launches"][0]
    assert (L["kf"], L["kt"], L["survivors"], L["non_survivors"], L["void"]) == (500, 500, 2000, 8000, 1506)
    total = L["valu_and_mfma"]
    print("parent: VALU %.2f M + MFMA %.2f M = %.2f M against %.2f M counted (%+.2f %%)"
          % (L["valu"] / 1e6, L["mfma"] / 1e6, total / 1e6, COUNTED_PARENT / 1e6, 100.0 * (total / COUNTED_PARENT - 1.0)))
    assert L["mfma"] == 10000 * 4 * 256               # (16 "from" tiles x 4 column tiles x 4 per wavefront)
    assert abs(total - COUNTED_PARENT) <= 0.05 * COUNTED_PARENT, total


@pytest.fixture(scope="module")
def now(tmp_path_factory):
    args = [x for m in MIXES for x in ("--mix", m)]
    r = _tool(*args)
    path = tmp_path_factory.mktemp("census") / "figures.json"
    path.write_text(json.dumps(r))
    return r, _tool("--figures", str(path), *args)


def test_figures_fed_back_give_the_same_tables(now):
    r, again = now
    for key in ("regions", "model_valu", "model_valu_repaired", "executed_model", "launches"):
        assert json.loads(json.dumps(r[key])) == again[key], key
    assert len(r["launches"]) == len(MIXES)


def test_a_launch_is_the_sum_of_its_parts(now):
    r, _ = now
    ex = r["executed_model"]
    ceil = lambda a, b: (a + b - 1) // b
    for L in r["launches"]:
        e, kf = L["per_wavefront"], L["kf"]
        assert e["prologue"] == ex["prologue"]["base"] + sum(l["valu"] * ceil(kf, l["rows_per_trip"]) for l in ex["prologue"]["loops"])
        c = ex["compaction"]
        assert e["compaction"] == c["always"] + sum(c["trips"][:ceil(kf, 256)]) + c["loop"] * ceil(kf, 256)
        assert e["outside_scan"] == e["prologue"] + e["handover"] + e["compaction"]
        wave = e["prologue"] + e["setup"] + e["groups"] + e["handover"] + e["compaction"]
        valu = (L["survivors"] * (4 * (wave + e["repair_per_wavefront"]) + e["tail_survivor"]) +
                L["non_survivors"] * (4 * wave + e["tail_non_survivor"]) + L["void"] * (4 * e["void_wavefront"] + e["tail_void"]))
        assert L["valu"] == valu and L["valu_and_mfma"] == valu + L["mfma"]
        assert L["mfma"] == (L["survivors"] + L["non_survivors"]) * 4 * e["mfma"]
    # the static model counts every loop outside the scan once: at K = 500 the executed count of a wavefront is that
    # plus the further trips, less what the static regions hold of other paths (void report, count of finite points)
    e500 = r["launches"][0]["per_wavefront"]
    static = r["model_valu"]["500"] if "500" in r["model_valu"] else r["model_valu"][500]
    executed = e500["prologue"] + e500["setup"] + e500["groups"] + e500["handover"] + e500["compaction"]
    print("K = 500: static model %d, executed %d per wavefront; outside the scan %d" % (static, executed, e500["outside_scan"]))
    assert abs(executed - static) <= 0.1 * static
