"""The population plan pinned on the CPU: the two host-only entries that report it
(edt_slerp_population_layout: the form and the per-component layout as JSON; edt_slerp_needed_table:
the needed-sums table's blocks and columns) give, over a recorded corpus of pair graphs, exactly
what tests/golden/population_plan.json holds — the library's own output when the fixture was
recorded (tests/golden/gen_population_plan.py), refusals (return code and message) included. The
plan is derived in one place in csrc/edt_slerp.hip; whatever changes there must leave every one of
these outputs as it is, or say why the fixture was recorded again."""
import ctypes
import json
import os

import pytest

from evolutionarydistributedtraining_amd import _lib as L

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "population_plan.json")
MAX_COLS = 36          # a triangle block over 8 members; the needed blocks of 8 members hold fewer


def record(case: dict, lib=None) -> dict:
    """What the two entries answer for one case {pairs, nmembers, nchunks}: "layout", the JSON for
    speculate = 1; "form0", the form for speculate = 0 (the rest of that JSON must equal "layout");
    "table", the needed table's outputs. A refusal is recorded as [return code, message]."""
    lib = lib or L.load_library()
    pairs, M, nch = case["pairs"], case["nmembers"], case["nchunks"]
    Q = len(pairs)
    fp = (ctypes.c_int32 * max(1, 2 * Q))(*[int(x) for p in pairs for x in p])
    lay = []
    for spec in (0, 1):
        buf = ctypes.create_string_buffer(16384)
        rc = lib.edt_slerp_population_layout(fp, Q, M, spec, buf, len(buf))
        lay.append(buf.value.decode() if rc == 0 else [rc, lib.edt_last_error().decode()])
    out = {"layout": lay[1], "form0": lay[0]}
    if isinstance(lay[0], str) and isinstance(lay[1], str):
        form = lambda js: json.loads(js)["form"]                                   # noqa: E731
        same = lay[0].replace(f'"form": "{form(lay[0])}"', f'"form": "{form(lay[1])}"') == lay[1]
        out["form0"] = form(lay[0]) if same else lay[0]          # the whole string where they differ elsewhere
    off = (ctypes.c_uint64 * 8)()
    nt = (ctypes.c_int32 * 8)()
    nc = ctypes.c_int32()
    cols = (ctypes.c_int32 * (2 * MAX_COLS))(*([-7] * (2 * MAX_COLS)))
    tot, scr = ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib.edt_slerp_needed_table(fp, Q, M, nch, off, nt, ctypes.byref(nc), cols, ctypes.byref(tot),
                                    ctypes.byref(scr))
    if rc:
        out["table"] = [rc, lib.edt_last_error().decode()]
    else:
        n = nc.value
        ncols = sum(nt[k] for k in range(n))
        out["table"] = {"ncomp": n, "block_off": [int(off[k]) for k in range(n)],
                        "block_nt": [int(nt[k]) for k in range(n)],
                        "col_members": [int(cols[x]) for x in range(2 * ncols)],
                        "table_doubles": int(tot.value), "scratch_doubles": int(scr.value)}
    return out


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_corpus_holds_what_it_is_meant_to(fixture):
    """nmembers 1..10, 0..20 children, both refusals and plans, every form and both stats layouts."""
    cases = fixture["cases"]
    assert len(cases) >= 250
    assert {c["case"]["nmembers"] for c in cases} >= set(range(1, 11))
    assert {len(c["case"]["pairs"]) for c in cases} >= set(range(0, 21))
    forms = set()
    kinds = set()
    for c in cases:
        if isinstance(c["want"]["layout"], str):
            js = json.loads(c["want"]["layout"])
            forms |= {js["form"], c["want"]["form0"]}
            kinds |= {k["stats_layout"] for k in js["components"]}
    assert forms == {"member-major", "co-located", "two-pass", "unsupported"}
    assert kinds == {"needed", "triangle"}
    assert any(isinstance(c["want"]["table"], list) for c in cases)
    assert any(isinstance(c["want"]["layout"], list) for c in cases)


def test_plan_outputs_equal_the_fixture(fixture):
    bad = []
    for c in fixture["cases"]:
        got = record(c["case"])
        if got != c["want"]:
            bad.append((c["name"], c["case"], {k: (got[k], c["want"][k]) for k in got if got[k] != c["want"][k]}))
    assert not bad, f"{len(bad)} of {len(fixture['cases'])} cases differ; first: {bad[0]}"
