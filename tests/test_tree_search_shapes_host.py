"""The CPU half of the trajectory tree search's shape sweep (tests/tree_search_cases.py): the table lands on both sides of every
comparison of mg_tree_plan_fit and of the 64 KiB test, the Python restatement of both LDS plans and of the ladder equals
csrc/mg_tree_plan.h (through tests/native/tree_plan_check, a program of its own), and every row is well conditioned for the oracle:
no two leaves' objectives lie within the comparison bound of each other, so a winner is never a coin toss."""
import os
import re
import subprocess

import numpy as np
import pytest

import tree_search_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def _source(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_constants_and_the_entry_points_match_the_source():
    header, src = _source("morphablegraphs_amd", "csrc", "mg_tree_plan.h"), _source("morphablegraphs_amd", "csrc", "mg_cluster_tree.hip")
    for name, value in (("MG_TREE_CHUNK", sc.CHUNK), ("MG_KD_GROUP", sc.KD_GROUP), ("MG_TREE_HENT_BYTES", sc.HENT), ("MG_TREE_KENT_BYTES", sc.KENT)):
        assert re.search(r"#define %s (\d+)\b" % name, header).group(1) == str(value), name
    assert "#define MG_TREE_LDS_MAX (160 * 1024 - 512)" in header and sc.LDS_MAX == 160 * 1024 - 512
    assert "#define MG_TREE_MAX_TRAJECTORIES %d" % sc.MAX_TRAJECTORIES in _source("include", "mg_hip.h")
    # the opt-in's comparison, and one gather and one ladder behind the searches and the query
    assert "if (lp.bytes > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in(MG_TREE_LDS_MAX, kernel));" in src
    assert "out->lds_opt_in = lp.bytes > 64 * 1024;" in src and "out->refused = lp.bytes > MG_TREE_LDS_MAX;" in src
    assert src.count("mg_tree_plan_fit(") == 2 and src.count("= mg_tree_gather(") == 2 and src.count("return mg_tree_planned(") == 2
    query = src[src.index('extern "C" int mg_cluster_tree_search_plan('):]
    query = query[:query.index("\n}\n")]
    assert "hip" not in query.replace("mg_hip", "") and "upload" not in query and "mg_tree_launch" not in query


def test_the_rows_claims_are_what_the_restated_plan_gives():
    for r in sc.ROWS:
        p = sc.row_plan(r)
        assert (p["state"], p["lds_opt_in"], p["refused"]) == (r["state"], r["over64"], False), (r["name"], p)
        assert 1 <= len(r["trajectories"]) <= sc.MAX_TRAJECTORIES
    for kind in sc.KINDS:
        assert sc.plan_fit(kind, sc.refused_shape(kind))["state"] == "refused"
    # every staging state for both tree kinds and both searches, each with an oracle row (all rows are flat trees)
    seen = {(r["state"], r["kind"], r["search"]) for r in sc.ROWS}
    assert seen == {(s, k, q) for s in sc.STATES for k in sc.KINDS for q in (0, 1)}
    assert {r["align"] for r in sc.ROWS} == {0, 1, 2}
    assert all(r["yardstick"] == "batched" or r["prim"] == "basis104" for r in sc.ROWS)
    # the root-row count beyond the root-path scorer: (L + rows) * 512 > 150 KiB (mg_traj_plan), so its row has the oracle alone
    L, NB = sc.PRIMS["basis104"]
    assert (L + 3 * NB + 4) * 512 > 150 * 1024 and all((l + 3 * nb + 4) * 512 <= 150 * 1024 for n, (l, nb) in sc.PRIMS.items() if n != "basis104")


def _side(boundary, r):
    """Which side of a ledger boundary the row lies on, from the plan's bytes at each comparison of the ladder"""
    c = sc.call_shape([sc.row_shape(r)]) if r["name"] != "refused" else sc.refused_shape(r["kind"])
    b = sc.ladder_bytes(r["kind"], c)
    final = sc.plan_fit(r["kind"], c)
    if boundary.startswith("bytes > 64 KiB"):
        want = {"everything staged": "all_staged", "W read": "w_memory", "polynomials read": "polynomials_memory", "root rows read": "root_rows_memory"}
        state = [v for k, v in want.items() if k in boundary][0]
        return None if final["state"] != state else ("above" if final["lds_bytes"] > sc.KB64 else "below")
    if "on the first plan" in boundary:
        return None if c["wrows"] == 0 else ("above" if b[0] > sc.LDS_MAX else "below")
    if "without W" in boundary:
        return None if (c["wrows"] > 0 and b[0] <= sc.LDS_MAX) else ("above" if b[1] > sc.LDS_MAX else "below")
    if "without the polynomials" in boundary:
        return None if b[1] <= sc.LDS_MAX else ("above" if b[2] > sc.LDS_MAX else "below")
    if "without the root rows" in boundary:
        return None if b[2] <= sc.LDS_MAX else ("above" if b[3] > sc.LDS_MAX else "below")
    if "st.wrows > 0" in boundary:
        return "below" if c["wrows"] == 0 else ("above" if b[0] > sc.LDS_MAX else None)
    raise AssertionError(boundary)


def _ledger_problems(rows):
    """What is wrong with the ledger over these rows: a listed row on the wrong side, or a side without a row for some kind and search"""
    problems = []
    refused = [dict(sc.REFUSED, kind=k, search=q, family="refused") for k in sc.KINDS for q in (0, 1)]
    for e in sc.LEDGER:
        for side in ("below", "above"):
            listed = [r for r in rows + refused if r["family"] in e[side]]
            for r in listed:
                if _side(e["boundary"], r) != side:
                    problems.append("%s: %s is not %s" % (e["boundary"], r["name"], side))
            for k in sc.KINDS:
                for q in (0, 1):
                    if not any(r["kind"] == k and r["search"] == q for r in listed):
                        problems.append("%s: nothing %s for %s, search %d" % (e["boundary"], side, k, q))
    return problems


def test_the_ledger_lands_on_both_sides_of_every_comparison():
    assert _ledger_problems(sc.ROWS) == []
    # ... and notices a row that goes missing: every family the ledger names is the only one of some side, or shares it
    named = {f for e in sc.LEDGER for side in ("below", "above") for f in e[side]} - {"refused"}
    assert named <= set(sc.families())
    for e in sc.LEDGER:
        for side in ("below", "above"):
            rest = [r for r in sc.ROWS if r["family"] not in e[side]]
            assert any(p.startswith(e["boundary"]) and ("nothing %s" % side) in p for p in _ledger_problems(rest)) or e[side] == ["refused"], (e["boundary"], side)
    # the distance from the boundary where the shapes can choose it: one step of what moves the plan
    for e in sc.LEDGER:
        if e["step"] is None:
            continue
        limit = sc.KB64 if "64 KiB" in e["boundary"] else sc.LDS_MAX
        index = 0 if ("64 KiB" in e["boundary"] or "first plan" in e["boundary"]) else (1 if "without W" in e["boundary"] else 2)
        for k in sc.KINDS:
            dist = {}
            for side in ("below", "above"):
                bs = [sc.ladder_bytes(k, sc.call_shape([sc.row_shape(r)]))[index] for r in sc.ROWS if r["family"] in e[side] and r["kind"] == k]
                dist[side] = min(abs(x - limit) for x in bs)
            assert dist["below"] < e["step"] and dist["above"] <= e["step"], (e["boundary"], k, dist)


def test_the_restated_plans_equal_the_header():
    """Every row's call, the refused shape and a grid of others through mg_tree_plan_fit itself: tests/native/tree_plan_check prints the
    fitted plan of the shapes on its command line (a program of its own, under the host sanitizers where the compiler has them)."""
    subprocess.check_call(["make", "-s", "-C", NATIVE, "-f", "tree_plan_check.mk", "tree_plan_check"])
    shapes = [(r["kind"], sc.call_shape([sc.row_shape(r)])) for r in sc.ROWS] + [(k, sc.refused_shape(k)) for k in sc.KINDS]
    rng = np.random.default_rng(4)
    for _ in range(200):
        kind = sc.KINDS[int(rng.integers(2))]
        traj = int(rng.integers(0, 5))
        shapes.append((kind, dict(L=int(rng.integers(1, 300)), nc=int(rng.integers(0, 260)), n_cand=int(rng.integers(1, 65)), children=int(rng.integers(0, 257)),
                                  depth=int(rng.integers(0, 65)), kd_children=int(rng.integers(0, 40)), kd_depth=int(rng.integers(0, 20)), traj=traj,
                                  wrows=int(rng.integers(0, 2)) * int(rng.integers(1, 1800)), cp_rows=int(rng.integers(0, 330)) if traj else 0,
                                  poly_doubles=int(rng.integers(0, 9000)) if traj else 0)))
    args = []
    for kind, c in shapes:
        args += [sc.KINDS.index(kind), c["L"], c["nc"], c["n_cand"], c["children"], c["depth"], c["kd_children"], c["kd_depth"], c["traj"], c["wrows"],
                 c["cp_rows"], c["poly_doubles"]]
    done = subprocess.run([os.path.join(NATIVE, "tree_plan_check")] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert done.returncode == 0, done.stdout.decode("utf-8", "replace")
    lines = done.stdout.decode().split("\n")[:len(shapes)]
    states = set()
    for (kind, c), line in zip(shapes, lines):
        p = sc.plan_fit(kind, c)
        assert [int(v) for v in line.split()] == [p["lds_bytes"], p["w_rows"], p["root_rows"], p["poly_doubles"], p["trajectory_slots"]], (kind, c, line, p)
        states.add(p["state"])
    assert states == set(sc.STATES) | {"refused"}


@pytest.mark.parametrize("name", sc.ROW_IDS)
def test_every_row_is_well_conditioned_for_the_oracle(name):
    """No two leaves' oracle objectives within twice the comparison bound of each other (the device's value may be off by the bound on
    either leaf), and every objective finite."""
    r = sc.BY_NAME[name]
    data, kf, trajs, latents = sc.row_inputs(r)
    assert len(kf) == r["n_keyframes"] and [len(t["control_points"]) - 1 for t in trajs] == [t["n_seg"] for t in r["trajectories"]]
    assert len(np.unique(latents, axis=0)) == r["n_leaves"]
    values, bounds = sc.oracle_objectives(data, kf, trajs, latents, r["align"], r["search"])
    assert np.all(np.isfinite(values))
    order = np.argsort(values)
    gaps = np.diff(values[order])
    assert np.all(gaps > 2.0 * np.maximum(bounds[order][1:], bounds[order][:-1])), (name, float(gaps.min()), float(bounds.max()))
