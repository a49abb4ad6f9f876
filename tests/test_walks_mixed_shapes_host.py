"""The mixed-population walk sweep without a device (tests/walks_mixed_shape_cases.py; the device half is
tests/test_gpu_walks_mixed_shapes.py).

1. The constants and the host decisions walks_frames_plan, walks_sample_plan and walks_time_plan restate are held to the text of
   csrc/mg_walks_mixed.hip and csrc/mg_timewarp_device.h.
2. Every row's plan gives the status the row expects; every route of DERIVED a row claims -- the five second trips among them -- follows
   from the plan's own rows, npairs, L and nch; the LDS edges sit exactly at their limits.
3. random_walks.assemble_walks_mixed_host -- the device sweep's reference -- is held to the oracle's control-point chain on every walk of
   every frame row of n_dim >= 7 that launches, warped rows at their own times, under tests/test_graph_walk_host.py's WALK_TOLERANCE with
   tests/test_walk_shapes_host.py's two input conditions (every heading's xz norm >= 0.1, no turn past pi - 0.05): asserted, no row skipped.
4. random_walks.walk_time_rows_host is held to FITPACK and to the 50-digit twin under timewarp_cases.time_tolerance; untimed rows are
   numpy.linspace's bits; every timed step's sample count is safe by timewarp_cases.MARGIN.
5. The sampler's component draw restated (random_walk_cases.walk_components): K = 1, every component of K = 7, -1 behind a walk's end.
6. MIXED_ROUTES holds every route the sweep was asked to take.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import random_walk_cases as rc
import timewarp_cases as tc
import walk_shape_cases as wc
import walks_mixed_shape_cases as mc
from morphablegraphs_amd import random_walks as rw
from morphablegraphs_amd.time_smoothing import WINDOW
from test_graph_walk_host import WALK_TOLERANCE, root_scale


def _csrc(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "morphablegraphs_amd", "csrc", name)).read()


def test_the_constants_are_the_sources():
    mixed, tw = _csrc("mg_walks_mixed.hip"), _csrc("mg_timewarp_device.h")
    for src, name, value in ((mixed, "MG_WALKS_TILE", mc.MG_WALKS_TILE), (mixed, "MG_WALKS_BLOCK", mc.MG_WALKS_BLOCK),
                             (mixed, "MG_WALKS_CHAIN_BLOCK", mc.MG_WALKS_CHAIN_BLOCK), (mixed, "MG_WALKS_SAMPLE_BLOCK", mc.MG_WALKS_SAMPLE_BLOCK),
                             (tw, "MG_TW_BLOCK", mc.MG_TW_BLOCK), (tw, "MG_TW_MAX_F", mc.MG_TW_MAX_F), (tw, "MG_TW_SMOOTH_W", mc.MG_TW_SMOOTH_W)):
        m = re.search(r"#define %s (\d+)\b" % name, src)
        assert m and int(m.group(1)) == value, name
    m = re.search(r"#define MG_WALKS_LDS_MAX \((\d+) \* 1024 - (\d+)\)", mixed)
    assert m and int(m.group(1)) * 1024 - int(m.group(2)) == mc.MG_WALKS_LDS_MAX == wc.MG_WALK_LDS_MAX
    m = re.search(r"#define MG_WALKS_SAMPLE_LDS_MAX \((\d+) \* 1024\)", mixed)
    assert m and int(m.group(1)) * 1024 == mc.MG_WALKS_SAMPLE_LDS_MAX
    half = int(re.search(r"#define MG_TW_SMOOTH_HALF (\d+)\b", tw).group(1))
    assert "#define MG_TW_SMOOTH_MID (MG_TW_BLOCK + 2 * MG_TW_SMOOTH_HALF)" in tw and "#define MG_TW_SMOOTH_LDS (MG_TW_SMOOTH_MID + 2 * MG_TW_SMOOTH_W)" in tw
    assert mc.MG_TW_SMOOTH_LDS == mc.MG_TW_BLOCK + 2 * half + 2 * mc.MG_TW_SMOOTH_W and WINDOW == mc.MG_TW_SMOOTH_W
    assert mc.MG_WALKS_TILE == wc.MG_WALK_TILE and mc.MG_WALKS_BLOCK == wc.MG_WALK_BLOCK and mc.MG_WALKS_CHAIN_BLOCK == wc.MG_WALK_CHAIN_BLOCK


def test_the_restated_decisions_are_the_sources():
    mixed = _csrc("mg_walks_mixed.hip")
    frames = mixed[mixed.index("static int mg_walks_frames_launch("):mixed.index('extern "C" int mg_walks_frames(')]
    for line in ("lmax = std::max(lmax, (int)p->L);", "rmax = std::max(rmax, (int)p->R);", "bool aligned_any = al != nullptr;",
                 "for (int64_t w = 0; w < n_walks && !aligned_any; w++) aligned_any = n_steps[w] > 1;", "MG_WALKS_REQUIRE(D >= 3 && (!aligned_any || D >= 7),",
                 "if (!aligned_any) {", "a.n_link = 0;", "} else if (joint == 0 && !sk) {", "a.n_link = 1; a.link[0] = 3;",
                 "const mg_plan_failure f = mg_aligning_quaternions(sk, joint, D, quats);", "a.n_link = (int32_t)quats.size();",
                 "const int64_t off = frame_offset ? frame_offset[ws] : next;", "step_tile[(size_t)ws] = (int32_t)walk_tiles;",
                 "walk_tiles += (len + MG_WALKS_TILE - 1) / MG_WALKS_TILE;", "MG_WALKS_REQUIRE(sp.first >= end,", "MG_WALKS_REQUIRE(end <= walk_stride,",
                 "walk_tile[(size_t)w + 1] = (int32_t)tiles;", "if (n_walks == 0) return MG_OK;",
                 "const size_t lds_f = ((size_t)rmax + lmax + MG_WALKS_TILE * 4) * 8 + MG_WALKS_TILE * 4;",
                 "const size_t lds_c = ((size_t)lmax + 5 * (3 + 4 * a.n_link) + 4) * 8 + 16;", "MG_REQUIRE_AS(lds_f <= MG_WALKS_LDS_MAX, MG_ERR_UNSUPPORTED,",
                 "MG_HIP_CHECK(mg_lds_opt_in_once(ctx, lds_bit, 160 * 1024,"):
        assert line in frames, line
    assert frames.index("MG_REQUIRE_AS(lds_f <= MG_WALKS_LDS_MAX") < frames.index("dt.upload(") < frames.index("hipLaunchKernelGGL(")      # refused before anything is written
    # the loops the second-trip rows are named for
    for line in ("for (int k = tid; k < st.L; k += MG_WALKS_CHAIN_BLOCK) s[k] =", "for (int e = tid; e < 5 * nch; e += MG_WALKS_CHAIN_BLOCK) {",
                 "const int nch = 3 + 4 * a.n_link;", "for (int k = tid; k < st.L; k += MG_WALKS_BLOCK) s[k] =", "const int rows = (imax + 4 - imin) * D, r0 = imin * D;",
                 "for (int e = tid; e < rows; e += MG_WALKS_BLOCK) {", "const int n = nf * D, odd = (int)(((uintptr_t)dst >> 3) & 1);",
                 "const int npairs = (n + odd + 1) >> 1;", "for (int p = tid; p < npairs; p += MG_WALKS_BLOCK) {"):
        assert line in mixed, line
    sample = mixed[mixed.index('extern "C" int mg_walks_sample_latents('):mixed.index("template <bool WARPED>")]
    for line in ("MG_WALKS_REQUIRE(!occurs[(size_t)k] || prims[k]->Lg <= ld,", "lgmax = std::max(lgmax, (int)prims[k]->Lg);",
                 "const size_t lds = (size_t)MG_WALKS_SAMPLE_BLOCK * (lgmax + 1) * 8;", "MG_REQUIRE_AS(lds <= MG_WALKS_SAMPLE_LDS_MAX, MG_ERR_UNSUPPORTED,",
                 "if (lds > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_WALKS_SAMPLE, 160 * 1024,",
                 "const unsigned grid = (unsigned)((rows + MG_WALKS_SAMPLE_BLOCK - 1) / MG_WALKS_SAMPLE_BLOCK);"):
        assert line in sample, line
    time = mixed[mixed.index("static int mg_walks_time_launch("):mixed.index('extern "C" int mg_walks_time_functions(')]
    for line in ("if (!occurs[(size_t)k]) continue;", "MG_WALKS_REQUIRE(p->L + p->Lt <= ld,", "MG_REQUIRE_AS(p->F >= 4 && p->F <= MG_TW_MAX_F, MG_ERR_UNSUPPORTED,",
                 "const double countf = (double)p->F * inv_speed;", "MG_WALKS_REQUIRE(countf >= 1.0,", "nd.count = (int32_t)countf;",
                 "const size_t lds = ((size_t)4 * fmax + (SMOOTH ? MG_TW_SMOOTH_LDS : 0)) * 8;", "dim3((unsigned)rows), dim3(MG_TW_BLOCK), lds,"):
        assert line in time, line


def _plan_or_status(make):
    try:
        return make(), mc.MG_OK
    except mc.Refused as e:
        return None, e.status


def test_every_row_has_the_status_its_plan_gives():
    for r in mc.MIXED_FRAME_ROWS:
        plan, status = _plan_or_status(lambda: mc.frame_plan(r))
        assert status == (r["expect"] if r["expect"] is not None else mc.MG_OK), r["name"]
        assert plan is None or plan["launched"] == bool(r["walks"])
    for r in mc.MIXED_TIME_ROWS:
        _, _, _, speed = mc.time_case(r)
        _, status = _plan_or_status(lambda: mc.time_plan(r, 4096, speed))
        assert status == (r["expect"] if r["expect"] is not None else mc.MG_OK), r["name"]
    for name in mc.SAMPLE_IDS:
        _, status = _plan_or_status(lambda: mc.sample_plan(name))
        assert status == mc.SAMPLE_REFUSED.get(name, mc.MG_OK), name
    # the refusals the tables have no row for, on the plans alone
    for make, status in ((lambda: mc.walks_sample_plan([(2, 5)], [[0]], 4), mc.INVALID), (lambda: mc.walks_sample_plan([(2, 5), (1, 9)], [[0]], 5), mc.MG_OK),
                         (lambda: mc.walks_time_plan([(2, 3, 0)], [[0]], 8, 4.0, 8), mc.INVALID), (lambda: mc.walks_time_plan([(2, 3, 0)], [[0]], 8, 2.0, 8), mc.MG_OK),
                         (lambda: mc.walks_time_plan([(3, 3, 1), (8, 3, 1)], [[1]], 8, 1.0, 8), mc.MG_OK), (lambda: mc.walks_time_plan([(3, 3, 1)], [[0]], 8, 1.0, 8), mc.UNSUPPORTED),
                         (lambda: mc.walks_frames_plan(mc.SMALL, 11, [[0, 1]], frame_offset=[[0, 5]]), mc.INVALID),
                         (lambda: mc.walks_frames_plan(mc.SMALL, 11, [[0, 1]], walk_stride=44), mc.INVALID), (lambda: mc.walks_frames_plan(mc.SMALL, 11, [[0, 3]]), mc.INVALID),
                         (lambda: mc.walks_frames_plan(mc.SMALL, 11, [[0, 1]], walk_stride=45), mc.MG_OK), (lambda: mc.walks_frames_plan(mc.SMALL, 11, [[0], []]), mc.INVALID),
                         (lambda: mc.walks_frames_plan(mc.SMALL, 11, [[0]], first_aligned=True, joint=1), mc.INVALID)):
        assert _plan_or_status(make)[1] == status


def test_the_claimed_routes_follow_from_the_plans():
    claimed = set()
    for r in mc.MIXED_FRAME_ROWS:
        if r["expect"] is not None:
            continue
        plan = mc.frame_plan(r)
        derived = mc.frame_routes(r, plan)
        assert r["routes"] & mc.DERIVED <= derived, (r["name"], sorted((r["routes"] & mc.DERIVED) - derived))
        claimed |= r["routes"] & mc.DERIVED
        # the per-walk tile prefix and the per-step tile starts: every tile is found again by the kernel's two bisections
        for t, tile in enumerate(plan.get("per_tile", [])):
            w = max(k for k in range(len(r["walks"])) if plan["walk_tile"][k] <= t)
            kt = t - plan["walk_tile"][w]
            i = max(k for k in range(len(r["walks"][w])) if plan["step_tile"][w][k] <= kt)
            assert (w, i, (kt - plan["step_tile"][w][i]) * mc.MG_WALKS_TILE) == (tile["walk"], tile["step"], tile["f0"]), (r["name"], t)
    assert claimed == mc.DERIVED
    by = mc.FRAME_BY_NAME
    # the five second trips, as numbers
    p = mc.frame_plan(by["second_trips"])
    assert max(t["rows"] for t in p["per_tile"]) == 9 * 39 > mc.MG_WALKS_BLOCK and max(t["npairs"][t["parity"]] for t in p["per_tile"]) >= 32 * 39 // 2 > mc.MG_WALKS_BLOCK
    assert p["lmax"] == 257 > mc.MG_WALKS_BLOCK and p["nch"] == 15 and 5 * 15 > mc.MG_WALKS_CHAIN_BLOCK >= 5 * 11 and p["chain_trips"] == 2
    assert sorted(L for L, _, _ in by["second_trips"]["shapes"]) == [8, 65, 257] and 65 > mc.MG_WALKS_CHAIN_BLOCK
    assert all(t["rows"] <= mc.MG_WALKS_BLOCK and max(t["npairs"]) <= mc.MG_WALKS_BLOCK for t in mc.frame_plan(by["D15_previous"])["per_tile"])
    assert [mc.frame_plan(by["chain_depth_%d" % d])["chain_trips"] for d in (1, 2, 3, 4, 7)] == [1, 1, 2, 2, 3]
    assert [mc.frame_plan(by["chain_depth_%d" % d])["n_link"] for d in (1, 2, 3, 4, 7)] == [1, 2, 3, 4, 7]
    assert mc.frame_plan(by["chain_max"])["n_link"] == wc.MG_MAX_CHAIN and mc.frame_plan(by["chain_unanimated_joint"])["link"] == [3, 7]
    assert len(wc.skeleton_of(by["chain_unanimated_joint"])[0]) == 3
    # the warped cp second trip comes from the times: the descending row's one tile holds all nine control-point rows of 39 channels
    p = mc.frame_plan(by["warped_second_trips"])
    assert p["per_tile"][0]["whole_spline"] and p["per_tile"][0]["rows"] == 9 * 39 and p["per_tile"][0]["nf"] == 31
    # mixed pitches: L = 1 and four control-point rows beside L = 257 and twelve rows; the small node before, between and after the large ones
    p = mc.frame_plan(by["pitches"])
    assert (p["lmax"], p["rmax"]) == (257, 12 * 11) and by["pitches"]["shapes"][0] == (1, 12, 4)
    assert [0, 1, 0, 2] in by["pitches"]["walks"] and [1, 0, 2, 0] in by["pitches"]["walks"]
    # LDS: the largest control-point block is exactly at the limit with walk_shape_cases' shapes, one latent more is past it
    p = mc.frame_plan(by["lds_largest"])
    assert p["lds_f"] == mc.MG_WALKS_LDS_MAX and p["rmax"] + p["lmax"] == wc.LDS_NB * wc.LDS_D + wc.LDS_L == 20328
    with pytest.raises(mc.Refused) as e:
        mc.frame_plan(by["lds_one_more"])
    assert e.value.status == mc.UNSUPPORTED and by["lds_one_more"]["shapes"][0][0] == wc.LDS_L + 1
    # padded tables, the population sizes, the empty call
    p = mc.frame_plan(by["population_65"])
    assert p["s_max"] == 4 and sorted(len(s) for s in by["population_65"]["walks"])[-2:] == [1, 4] and (rc.tables(by["population_65"]["walks"])[0] == -1).sum() == 64 * 3
    assert {len(r["walks"]) for r in mc.MIXED_FRAME_ROWS} >= {0, 1, 2, 5, 64, 65}
    p = mc.frame_plan(by["no_walks"])
    assert not p["launched"] and p["tiles"] == 0 and p["walk_tile"] == [0]
    # offsets with gaps and out of order
    offs = by["offsets_with_gaps"]["offsets"]
    assert any(o[0] > o[-1] for o in offs if len(o) > 1) and any(o[0] < o[-1] for o in offs if len(o) > 1) and min(min(o) for o in offs) == 3


def test_the_warped_rows_time_rows_cover_their_list():
    names = [r["name"] for r in mc.MIXED_FRAME_ROWS if r["warped"]]
    assert set(names) >= {"warped_second_trips", "warped_chain_depth_3", "warped_pitches"} and any(mc.FRAME_BY_NAME[n]["D"] % 2 == 0 for n in names)
    seen, on_knot, repeated, ends = set(), 0, 0, 0
    for name in names:
        row = mc.FRAME_BY_NAME[name]
        lengths, times = mc.warped_times(row)
        plan = mc.frame_plan(row)
        assert plan["t_cap"] == max(max(l) for l in lengths)
        for w, seq in enumerate(row["walks"]):
            for i, k in enumerate(seq):
                _, F, NB = row["shapes"][k]
                t, knots = times[w][i], mc.synthetic.cubic_b_spline_knots(NB, F)
                assert len(t) == lengths[w][i] and t.min() >= 0.0 and t.max() <= F - 1.0
                seen.add(len(t))
                on_knot += int(np.isin(t, knots[4:NB]).any())
                repeated += int(len(np.unique(t)) < len(t))
                ends += int(0.0 in t and F - 1.0 in t)
        assert any(t["whole_spline"] and t["nf"] in (31, 32) for t in plan["per_tile"]), name
        first = times[0][0]
        assert (np.diff(first) <= 0).all() and first[0] == row["shapes"][row["walks"][0][0]][1] - 1.0 and first[-1] == 0.0
    assert seen == {1, 2, 31, 32, 33, 64, 65} and min(on_knot, repeated, ends) >= len(names)


LAUNCHED = [r["name"] for r in mc.MIXED_FRAME_ROWS if r["expect"] is None and r["D"] >= 7 and r["walks"]]


@pytest.mark.parametrize("name", LAUNCHED)
def test_assemble_walks_mixed_host_is_the_oracles_chain_on_every_row(name):
    r = mc.FRAME_BY_NAME[name]
    models, P, alignment, hip_sk, skel, prev = mc.frame_case(r)
    node_of, n_steps = mc.frame_tables(r)
    lengths, times, _, _ = mc.frame_layout(r)
    frames, offsets, transforms = rw.assemble_walks_mixed_host(models, node_of, n_steps, P, alignment, hip_sk, times=times)
    node = r["node"] if r["kind"] == "previous" else skel[0][0][0]
    ref_dir = r["ref_dir"] if r["kind"] == "previous" else (0.0, 0.0, 1.0)
    bound = r["bound"] if r["bound"] is not None else WALK_TOLERANCE
    worst_row = 0.0
    for w, seq in enumerate(r["walks"]):
        want_len = sum(lengths[w]) if r["warped"] else sum(r["shapes"][k][1] for k in seq)
        assert frames[w].shape == (want_len, r["D"]) and not np.isnan(frames[w]).any()
        ref, least, widest = mc.oracle_walk([models[k] for k in seq], mc.walk_latents(r, P, w), r["kind"], node, skel, prev, ref_dir, None if times is None else times[w])
        assert least >= 0.1, "a heading of row %s, walk %d is badly conditioned: %g" % (name, w, least)
        assert widest <= np.pi - 0.05, "a step of row %s, walk %d turns by %g: the oracle's half angle is the other root quaternion" % (name, w, widest)
        worst = float(np.max(np.abs(frames[w] - ref))) / root_scale(ref)
        worst_row = max(worst_row, worst)
        assert worst <= bound, (name, w, worst)
        assert np.isnan(transforms[w, len(seq):]).all() and np.allclose(transforms[w, :len(seq), 0] ** 2 + transforms[w, :len(seq), 1] ** 2, 1.0, atol=1e-12)
    print("row %s: worst disagreement %.3g of the root scale (bound %.3g)" % (name, worst_row, bound))


def test_every_row_is_held_to_the_oracle_or_to_the_back_projection():
    rest = [r for r in mc.MIXED_FRAME_ROWS if r["name"] not in LAUNCHED]
    assert all(r["expect"] is not None or not r["walks"] or (r["D"] < 7 and r["kind"] == "none" and all(len(s) == 1 for s in r["walks"])) for r in rest)
    assert len({r["seed"] for r in mc.MIXED_FRAME_ROWS}) == len(mc.MIXED_FRAME_ROWS)
    assert all(r["bound"] is None for r in mc.MIXED_FRAME_ROWS)          # no row needed a bound of its own: every one is under WALK_TOLERANCE


# ---- the time rows ------------------------------------------------------------------------------------------------------------------
TIME_LAUNCHED = [r["name"] for r in mc.MIXED_TIME_ROWS if r["expect"] is None]


@pytest.mark.parametrize("name", TIME_LAUNCHED)
def test_walk_time_rows_host_against_the_twin(name):
    r = mc.TIME_BY_NAME[name]
    jsons, shapes, P, speed = mc.time_case(r)
    node_of, n_steps = rc.tables(r["walks"])
    assert r["ld"] > max(L + Lt for _, L, Lt in shapes)
    rows = rw.walk_time_rows_host(jsons, node_of, n_steps, P.astype(np.float64), speed)
    want = mc.time_reference(name)
    worst = 0.0
    for (w, i), ref in want.items():
        got = rows[w][i]
        if not ref["timed"]:
            assert got.shape == ref["row"].shape and np.array_equal(got.view(np.uint64), ref["row"].view(np.uint64)), (w, i)
            continue
        assert min(ref["margins"]) >= tc.MARGIN, "row %s, step %s: the sample count is not safe (%g, %g)" % ((name, (w, i)) + ref["margins"])
        assert len(got) == len(ref["row"]) == len(ref["twin"]) == tc.sample_count(ref["canonical"], speed) + 2
        worst = max(worst, float(np.max(np.abs(got - ref["twin"]))) / ref["tol"])
        assert np.max(np.abs(got - ref["twin"])) <= ref["tol"] and np.max(np.abs(got - ref["row"])) <= ref["tol"], (w, i)
    print("row %s: worst |host - twin| / tolerance %.3g" % (name, worst))
    if r["sized"] is not None:
        assert len(rows[0][0]) == r["sized"]


def test_the_time_rows_cover_their_list():
    R = mc.MIXED_TIME_ROWS
    used = lambda r: {r["nodes"][k] for seq in r["walks"] for k in seq if not (isinstance(r["nodes"][k], tuple) and r["nodes"][k][0] == "json")}
    launched = [r for r in R if r["expect"] is None]
    assert set().union(*[used(r) for r in launched]) >= set(tc.MODELS) | set(tc.CONSTANT)
    for name, spec in tc.CONSTANT.items():
        assert mc.TIME_BY_NAME["constant_" + name]["speed"] == spec[5]
    assert {r["speed"] for r in launched if r["speed"] is not None} >= set(tc.SPEEDS) and {np.dtype(r["dtype"]).name for r in launched} == {"float32", "float64"}
    counts = {int(mc.UNTIMED[nd] * (1.0 / r["speed"])) for r in launched if r["speed"] is not None for nd in used(r) if nd in mc.UNTIMED}
    assert counts >= {1, 2, 64, 65}
    assert all({len(s) for s in r["walks"]} <= {1, 2, 3} for r in R) and any(r["short"] for r in R)
    mixes = [any(r["nodes"][k] in mc.UNTIMED for k in seq) and any(r["nodes"][k] not in mc.UNTIMED for k in seq) for r in launched for seq in r["walks"]]
    assert sum(mixes) >= 10
    assert {r["sized"] for r in R if r["sized"] is not None} == {WINDOW - 1, WINDOW, WINDOW + 1} and sum(bool(r["smooth"]) for r in R) >= 5
    assert mc.TIME_ROUTES >= {"refused:time_F3", "refused:time_F2049", "refused:time_ld", "time:unsupported_node_does_not_occur", "time:one_short"}


# ---- the sampler's rows -------------------------------------------------------------------------------------------------------------
def test_the_sampler_rows_sit_on_both_sides_of_their_limits():
    assert mc.LG_LARGEST == 299 and mc.walks_sample_plan([(1, 299)], [[0]], 299)["lds"] == mc.MG_WALKS_SAMPLE_LDS_MAX
    with pytest.raises(mc.Refused) as e:
        mc.walks_sample_plan([(1, 300)], [[0]], 300)
    assert e.value.status == mc.UNSUPPORTED == mc.SAMPLE_REFUSED["one_past_the_largest"]
    assert not mc.walks_sample_plan([(1, 127)], [[0]], 127)["opt_in"] and mc.walks_sample_plan([(1, 128)], [[0]], 128)["opt_in"]
    assert mc.sample_plan("Lg127_65_rows")["lds"] == mc.KB64 and mc.sample_plan("Lg128_129_rows")["opt_in"] and mc.sample_plan("largest")["lds"] == mc.MG_WALKS_SAMPLE_LDS_MAX
    assert [mc.sample_plan(n)["grid"] for n in ("narrow_63_rows", "narrow_64_rows_wide_ld", "Lg127_65_rows", "Lg128_129_rows")] == [1, 1, 2, 3]
    assert [mc.sample_plan(n)["rows"] for n in ("narrow_63_rows", "narrow_64_rows_wide_ld", "Lg127_65_rows", "Lg128_129_rows")] == [63, 64, 65, 129]


@pytest.mark.parametrize("name", [n for n in mc.SAMPLE_IDS if n not in mc.SAMPLE_REFUSED])
def test_the_component_draw_of_every_sampler_row(name):
    mixtures, walks, ld, seed = mc.MIXED_SAMPLE_ROWS[name]
    node_of, n_steps = rc.tables(walks)
    weights = [mc.sample_model(K, Lg)["gmm_weights"] for K, Lg in mixtures]
    comp = rc.walk_components(weights, node_of, n_steps, seed)
    assert np.array_equal(comp == -1, node_of == -1)
    for k, (K, _) in enumerate(mixtures):
        drawn = set(comp[node_of == k].tolist())
        assert drawn == set(range(K)), "row %s: node %d of %d components draws %s at seed %d" % (name, k, K, sorted(drawn), seed)
    assert len(set(mixtures)) == len(mixtures)


def test_the_routes_hold_everything_the_sweep_was_asked_for():
    want = {"D:%d" % D for D in (3, 4, 6, 7, 8, 11, 12, 15)} | {"mode:%s" % m for m in ("none", "previous", "start_pose")} | {"lat:float32", "lat:float64", "steps:1_2_3"}
    want |= {"chain:depth_%d" % d for d in (1, 2, 3, 4, 7)} | {"chain:max_links", "refused:chain", "chain:unanimated_joint", "ref_dir:x", "ref_dir:oblique", "chain:no_links"}
    want |= {"frames:cp_second_trip", "frames:store_second_trip", "frames:latents_second_trip", "chain:entries_second_trip", "chain:latents_second_trip"}
    want |= {"frames:below_lmax_rmax", "frames:both_parities", "frames:even_D", "offsets:gaps_out_of_order", "frames:last_tile_one_frame", "frames:last_tile_32_frames",
             "frames:lds_largest", "refused:lds", "refused:D_below_7", "tables:padded_behind_the_ends", "frames:root_is_the_whole_row", "frames:unaligned"}
    want |= {"walks:%d" % n for n in (0, 1, 2, 5, 64, 65)}
    want |= {"warped:%s" % b for b in ("second_trips", "chain_depth_3", "pitches")} | {"warped:lengths", "warped:on_knots", "warped:repeated_times", "warped:whole_spline_tile"}
    want |= {"time:model_F%d_Lt%d" % key for key in tc.MODELS} | {"time:constant_" + name for name in tc.CONSTANT} | {"time:speed_%g" % s for s in tc.SPEEDS}
    want |= {"time:untimed_count_%d" % c for c in (1, 2, 64, 65)} | {"time:lat_float32", "time:lat_float64", "time:one_short", "time:smoothed"}
    want |= {"time:smoothed_%d_samples" % T for T in (14, 15, 16)} | {"refused:time_F3", "refused:time_F2049", "refused:time_ld", "time:unsupported_node_does_not_occur"}
    want |= {"sample:Lg_%d" % Lg for Lg in (1, 3, 4, 5, 127, 128, 299)} | {"sample:K_%d" % K for K in (1, 2, 7)} | {"sample:rows_%d" % n for n in (63, 64, 65, 129)}
    want |= {"sample:float64", "sample:float32", "sample:ld_equal", "sample:ld_wider", "sample:comp_given", "sample:comp_null", "sample:opt_in", "sample:plain_lds",
             "sample:lds_largest", "refused:sample_lds"}
    assert want <= mc.MIXED_ROUTES, sorted(want - mc.MIXED_ROUTES)
    assert any(r["D"] % 2 == 0 and r["warped"] for r in mc.MIXED_FRAME_ROWS)
    for D in (7, 8, 11, 12, 15):
        assert {(r["kind"]) for r in mc.MIXED_FRAME_ROWS if r["name"].startswith("D%d_" % D)} == {"none", "previous", "start_pose"}
        assert {np.dtype(r["dtype"]).name for r in mc.MIXED_FRAME_ROWS if r["name"].startswith("D%d_" % D)} == {"float32", "float64"}
        assert all({len(s) for s in r["walks"]} >= {1, 2, 3} for r in mc.MIXED_FRAME_ROWS if r["name"].startswith("D%d_" % D))
