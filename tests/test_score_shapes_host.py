"""The keyframe scorers' sweep without a device (tests/score_shape_cases.py; the device half is tests/test_gpu_score_shapes.py).

1. score_route is held to the C text of csrc/mg_score_route.h line by line, the launch code to calling it (no second copy of the
   decision), set_rows to csrc/mg_constraint_image.h, k_steps to mg_primitive_create, the update's limit to mg_launch_set_params.
2. ROWS lands on both sides of every comparison of the route, and every row takes the kernels it claims.
3. Every (kernel, latent dtype, what is written) combination the dispatch can select is claimed by some row.
4. The reference-only conditions, on the oracle alone, for every row: no cosine fed to acos within 1e-6 of +-1, no heading or
   direction norm below 1e-6, and the two smallest errors of every argmin row differ unless the row is a tie on purpose.  The seeds are
   chosen so that no row needs excluding; the device tests skip nothing.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import score_shape_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _csrc(name):
    return _source("morphablegraphs_amd", "csrc", name)


def test_restatement_matches_the_source():
    route, score, host, image = _csrc("mg_score_route.h"), _csrc("mg_score.hip"), _csrc("mg_host.hip"), _csrc("mg_constraint_image.h")
    header, hostdefs = _source("include", "mg_hip.h"), _csrc("mg_hostdefs.h")
    for src, name, value in ((route, "MG_SCORE_WIDE_MIN_B", sc.MG_SCORE_WIDE_MIN_B), (score, "MG_SET_PARAMS_MAX", sc.MG_SET_PARAMS_MAX),
                             (header, "MG_MAX_CHAIN", sc.MG_MAX_CHAIN), (header, "MG_MAX_POSE_POINTS", sc.MG_MAX_POSE_POINTS), (hostdefs, "MG_MAX_KK", sc.MG_MAX_KK),
                             (score, "MG_SC_CANDS", 64), (score, "MG_SC_WAVES", 4), (header, "MG_SCORE_KERNEL_VALU", 0), (header, "MG_SCORE_KERNEL_TILE", 1),
                             (header, "MG_SCORE_KERNEL_WIDE", 2)):
        m = re.search(r"#define %s (\d+)\b" % name, src)
        assert m and int(m.group(1)) == value, name
    assert sc._capi.MG_SCORE_KERNELS == ("valu", "tile", "wide")
    # mg_score_route_of, in the order score_route states it
    lines = ("const bool packed = has_wpack && !force_valu && mg_dispatch_kk(KK, false, [](auto) { return true; });",
             "const bool wide = kernel_opt == 2 || (kernel_opt == 0 && B >= MG_SCORE_WIDE_MIN_B);",
             "const size_t wide_lds = (size_t)4 * 64 * ((size_t)RT * 16 + 1) * 8;",
             "if (wide && wide_lds <= 64 * 1024) {",
             "const int64_t grid = (B + 255) / 256;",
             "if (grid <= 0x7fffffff) { *out = {MG_SCORE_KERNEL_WIDE, wide_lds, false, grid}; return MG_SCORE_ROUTE_OK; }",
             "fits = false;",
             "const size_t lds = (size_t)4 * (16 * ((size_t)RT * 16 + 1) + (size_t)std::max(n, 1) * 16) * 8;",
             "if (fits && lds <= 150 * 1024 && grid <= 0x7fffffff) { *out = {MG_SCORE_KERNEL_TILE, lds, lds > 64 * 1024, grid}; return MG_SCORE_ROUTE_OK; }",
             "const size_t lds = ((size_t)64 * ((size_t)L + 1) + (size_t)std::max(n, 1) * 64) * 8;",
             "*out = {MG_SCORE_KERNEL_VALU, lds, lds > 64 * 1024, grid};",
             "if (lds > 150 * 1024) return MG_SCORE_REFUSED_LDS;",
             "if (grid > 0x7fffffff) return MG_SCORE_REFUSED_SAMPLES;")
    at = 0
    for line in lines:
        assert line in route[at:], line
        at = route.index(line, at)
    assert route.count("64 * 1024") == 3 and route.count("150 * 1024") == 2 and route.count("MG_SCORE_WIDE_MIN_B") == 2
    assert route.count("const int64_t grid = (B + 63) / 64;") == 2
    assert "hip_runtime" not in route and "hipLaunch" not in route            # no HIP call: the native check compiles it alone
    # the launch code and the plan call it, and hold no copy of the decision
    body = score[score.index("static int mg_launch_score_mfma_kk("):score.index("// New constraint parameters for an existing set")]
    assert body.count("mg_score_route_of(") == 1 and body.count("mg_score_route_for(p, cs,") == 2
    for word in ("64 * 1024", "150 * 1024", "MG_SCORE_WIDE_MIN_B", "0x7fffffff", "+ 63) / 64", "+ 255) / 256"):
        assert word not in body, word
    for line in ("return mg_score_route_of(p->KK, p->L, cs->RT, cs->n, B, p->ctx->opt[MG_OPT_SCORE_KERNEL], p->ctx->opt[MG_OPT_FORCE_VALU_SCORE], cs->d_Wpack != nullptr, r);",
                 "if (r.opt_in) MG_HIP_CHECK(mg_lds_opt_in(160 * 1024, kernel));",
                 'mg_set_error("mg_score_constraints: n_components %d x %d constraints too large for LDS", p->L, cs->n);',
                 'mg_set_error("mg_score_constraints: too many samples");',
                 "out->kernel = r.kernel; out->lds_opt_in = r.opt_in ? 1 : 0; out->rows = cs->rows; out->row_tiles = cs->RT;"):
        assert line in body, line
    assert body.count("if (r.opt_in)") == 2 and "mg_score_mfma64_kernel<KK, LAT_F64, OUT_F64>), dim3((int)r.grid), dim3(256), r.lds" in body
    # lanes past the batch end take the last candidate's alignment row (both kernels; the wide kernel's lanes stop at ncand)
    assert "const int64_t cand = b0 + (lane < ncand ? lane : ncand - 1);" in score and "b0 + (cand < ncand ? cand : ncand - 1));" in score
    assert "if (lane < ncand) {" in score
    # the update's limit
    for line in ("struct mg_set_params_args { double v[MG_SET_PARAMS_MAX]; };", "if (n_par + n_align > MG_SET_PARAMS_MAX) {"):
        assert line in score, line
    assert "mg_launch_set_params(cs->prim->ctx, values.data(), n * 8, al ? 7 : 0, cs->d_par, al ? cs->d_align + 1 : nullptr);" in host
    # the rows of a set and whether it has the packed image
    for line in ("im.nch = std::min(7, D);", "const size_t r0 = add_rows(c, im.nch);", "const int block = 3 + 4 * n_slots, blocks = pc.has_velocity ? 2 : 1;",
                 "const int m = (int)chain.size() - 1 + ((r.own_quat || relative) ? 1 : 0), m2 = r.second ? (int)chain2.size() - 1 : 0;",
                 "const int q = std::max(m, 1), q2 = r.second ? std::max(m2, 1) : 0, root = r.root_rows ? 3 : 0;", "const size_t r0 = add_rows(c, root + 4 * q + 4 * q2);",
                 "add_rows(n, al ? 3 + 4 * (int)al_chain.size() : 0)", "if (KK > 0 && rows_total > 0) {", "im.RT = (int32_t)((rows_total + 15) / 16);",
                 'MG_REQUIRE(m <= MG_MAX_CHAIN, "mg_constraint_set_create_fk: constraint %d: chain of %d joints exceeds %d", c, m, MG_MAX_CHAIN);'):
        assert line in image, line
    assert "p->KK = (L <= 4 * MG_MAX_KK) ? (((L + 3) / 4 + 1) / 2) * 2 : 0;" in _csrc("mg_primitive_image.h")


def _kernel(row, label, B=None):
    p = sc.row_plan(sc.BY_NAME[row], max(sc.BY_NAME[row]["batches"]) if B is None else B, label)
    return p["kernel"] + (":opt_in" if p["lds_opt_in"] else "")


def test_the_rows_land_on_both_sides_of_every_comparison():
    R = sc.BY_NAME
    rows = {name: sc.row_rows(r) for name, r in R.items()}
    # rows 16 / 17 under option 2, and the wide sets with content
    assert (rows["wide16"], rows["tile17"], rows["wide14"], rows["wide15"], rows["wide14_aligned"], rows["wide15_d3"]) == (16, 17, 14, 15, 14, 15)
    assert len(R["wide16"]["cons"]) == 4 and {c["type"] for c in R["wide16"]["cons"]} == {"joint_orientation"}
    assert [c["type"] for c in R["wide15"]["cons"]] == ["look_at", "joint_orientation", "value_heading"]
    assert R["wide15_d3"]["D"] == 3 and len(R["wide15_d3"]["cons"]) == 5 and R["wide14_aligned"]["chained"] and R["wide14_aligned"]["align"] == "previous"
    assert _kernel("wide16", "wide") == "wide" and sc.score_route(8, 17, 2, 65, kernel_opt=2)["kernel"] == "tile"
    with pytest.raises(KeyError):
        sc.row_plan(R["tile17"], 65, "nothing")
    assert "wide" not in [l for l, _, _ in sc.routes_of(R["tile17"])] and sc.score_route(8, rows["tile17"], 2, 65, kernel_opt=2)["kernel"] == "tile"
    for name in ("wide14", "wide16", "wide15", "wide14_aligned", "wide14_aligned_dir", "wide15_d3", "n1", "wide_ld"):
        for B in R[name]["batches"]:
            p = sc.row_plan(R[name], B, "wide")
            assert p["kernel"] == "wide" and p["lds_bytes"] == 34816 and p["workgroups"] == (B + 255) // 256 and p["row_tiles"] == 1, (name, B)
    # the batch sizes: tiles of a wide wave past the end, a one-row tile, waves that return at once, a second workgroup
    assert set(R["wide14"]["batches"]) == {1, 15, 16, 17, 48, 49, 63, 64, 65, 255, 256, 257}
    for name in ("tile17", "n3", "L65"):
        assert set(R[name]["batches"]) == {1, 15, 16, 17, 63, 64, 65, 257}
    assert R["tile17"]["claims"] >= {"tile", "valu"} and _kernel("L65", "tile") == "valu" and R["L65"]["L"] == 65 and sc.k_steps(65) == 0
    assert all(set(R[name]["batches"]) == {17, 65} for name in R if R[name]["chained"])
    # the automatic switch
    assert sc.AUTO_B == (49151, 49152) and [sc.row_plan(sc.AUTO_ROW, B, "auto")["kernel"] for B in sc.AUTO_B] == ["tile", "wide"]
    # n = 0, 1, 3, 4, 5
    assert [len(R[k]["cons"]) for k in ("n0", "n1", "n3", "n4", "n5")] == [0, 1, 3, 4, 5]
    assert {_kernel("n0", label) for label in ("tile", "wide", "valu", "auto")} == {"valu"} and sc.row_plan(R["n0"], 65, "auto")["rows"] == 0
    # tile LDS: 64 KiB between n and n + 1, 150 KiB likewise, past it the VALU kernel without an error
    a, b = sc.TILE_64K_N, sc.TILE_150K_N
    tile = lambda n: sc.row_plan(R["tile_lds_n%d" % n], 17, "tile")
    assert (a, b) == (31, 74) and tile(a)["lds_bytes"] == sc.KB64 and not tile(a)["lds_opt_in"] and tile(a + 1)["lds_opt_in"] and tile(a + 1)["kernel"] == "tile"
    assert tile(b)["kernel"] == "tile" and tile(b)["lds_bytes"] <= sc.KB150 < 512 * (16 * 15 + 1 + b + 1) and tile(b + 1)["kernel"] == "valu" and not tile(b + 1)["lds_opt_in"]
    # VALU LDS
    a, b = sc.VALU_64K_N, sc.VALU_150K_N
    valu = lambda n: sc.row_plan(R["valu_lds_n%d" % n], 17, "auto")
    assert (a, b) == (62, 234) and valu(a)["lds_bytes"] == sc.KB64 and not valu(a)["lds_opt_in"] and valu(a + 1)["lds_opt_in"] and valu(b)["lds_bytes"] == sc.KB150
    with pytest.raises(sc.Refused, match="too large for LDS") as e:
        valu(b + 1)
    assert e.value.status == sc.MG_ERR_UNSUPPORTED == R["valu_lds_n%d" % (b + 1)]["expect"]
    # ld > L, the update's limit, the chains
    assert R["wide_ld"]["ld_extra"] > 0 and R["wide_ld_L65"]["ld_extra"] > 0 and R["wide_ld_L65"]["L"] == 65
    assert sc.UPDATE_N * 8 <= sc.MG_SET_PARAMS_MAX < (sc.UPDATE_N + 1) * 8 and sc.UPDATE_N == 62
    line = sc.line_skeleton()
    assert len(line[0]) == 33 and len(line[1]) == 31 and sc.chain_links(line, "j32") == sc.MG_MAX_CHAIN and sc.LINE_D == 127
    assert sc.chain_links(sc.line_skeleton(34), "j33") == sc.MG_MAX_CHAIN + 1 == sc.chain_links(R["chain33"]["skel"], R["chain33"]["cons"][0]["joint"])
    assert R["chain33"]["expect"] == sc.MG_ERR_INVALID_ARGUMENT
    assert sc.chain_links(line, R["chain31_relative"]["cons"][0]["joint"]) + 1 == sc.MG_MAX_CHAIN and R["chain31_relative"]["cons"][0]["offset"] is not None
    assert rows["chain32"] == 3 + 4 * 32 and rows["chain32_midpoint"] == 3 + 4 * 32 + 4 * 3 and rows["pose1"] == 127 and rows["pose64_velocity"] == 254
    assert {(len(R[k]["cons"][0]["joints"]), R[k]["cons"][0]["velocity"] is not None) for k in R if k.startswith("pose")} == {(1, False), (1, True), (64, False), (64, True)}
    # every row takes the kernels it claims
    for name, r in R.items():
        if r["expect"] is not None:
            continue
        got = {_kernel(name, label, B) for label, _, _ in sc.routes_of(r) for B in r["batches"]}
        want = {c for c in r["claims"] if c != "valu:fallthrough"}
        assert want <= got, (name, want, got)
        if "valu:fallthrough" in r["claims"]:
            assert _kernel(name, "tile") == "valu"
        if "wide" in r["claims"]:
            assert all(sc.row_plan(r, B, "wide")["kernel"] == "wide" for B in r["batches"])
    assert len({r["seed"] for r in sc.ROWS}) == len(sc.ROWS)


def test_every_combination_the_dispatch_can_select_is_claimed():
    claimed = set().union(*[sc.claimed_combos(r) for r in sc.ROWS])
    assert claimed == sc.COMBOS, sorted(sc.COMBOS - claimed)
    specials = set().union(*[r["claims"] for r in sc.ROWS]) - {"wide", "tile", "valu"}
    assert specials | {"auto:tile", "auto:wide"} == sc.SPECIALS
    # the chained entry reaches all three kernels
    assert {k for r in sc.ROWS if r["chained"] for (k, _, o) in sc.claimed_combos(r) if o == "res_align_cand"} == {"wide", "tile", "valu"}


@pytest.mark.parametrize("name", [r["name"] for r in sc.ROWS if r["oracle"] is not None])
def test_the_rows_inputs_are_well_conditioned(name):
    row = sc.BY_NAME[name]
    worst_cos, least = sc.conditioning(row, sc.latents(row))
    print("row %s: largest |cosine| %.9f, smallest norm %.3g" % (name, worst_cos, least))
    assert worst_cos <= 1.0 - 1e-6 and least >= 1e-6


def test_the_automatic_switch_batch_is_well_conditioned():
    row = sc.AUTO_ROW
    assert sc.row_rows(row) == 14 and row["L"] <= 8
    worst_cos, least = sc.conditioning(row, sc.auto_latents(sc.AUTO_B[1]))
    print("largest |cosine| %.9f, smallest norm %.3g over %d candidates" % (worst_cos, least, sc.AUTO_B[1]))
    assert worst_cos <= 1.0 - 1e-6 and least >= 1e-6


def test_per_candidate_headings_are_the_numbers_the_record_would_hold():
    for row in sc.ROWS:
        if row["chained"]:
            A = sc.align_cand_of(row, 65)
            assert np.all(np.sqrt(A[:, 0] * A[:, 0] + A[:, 1] * A[:, 1]) == 1.0) and len({tuple(a) for a in A}) == 65


def test_argmin_rows_have_one_winner_unless_they_tie_on_purpose():
    names = set(sc.ARGMIN_CASES)
    assert {"tie_one_thread", "tie_across_lanes", "tie_across_waves", "negative_zero_first", "positive_zero_first", "all_nan", "all_inf", "one_negative_inf"} <= names
    assert all("distinct_%d" % n in names and "min_first_%d" % n in names and "min_last_%d" % n in names for n in sc.ARGMIN_SIZES)
    assert "min_at1024_1025" in names and "min_at1024_2049" in names and "tie_ends_2049" in names
    for name, (v, tie) in sc.ARGMIN_CASES.items():
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v, equal_nan=True), name       # both value dtypes hold the case
        finite = np.sort(v[~np.isnan(v)])
        if not tie:
            assert len(finite) == 1 or finite[0] < finite[1], name
        else:
            assert len(finite) == 0 or finite[0] == finite[1], name
        i, m = sc.c_oracle.first_min_argmin(v)
        j, m2 = sc.orc.first_min_argmin(v)
        assert i == j and (m == m2 or (np.isinf(m) and np.isinf(m2))), name
        if name.startswith("tie_") or name.endswith("zero_first"):
            assert i == int(np.flatnonzero(v == np.nanmin(v))[0]), name
    # the two smallest errors of the best-candidate rows differ (the tie row of the device test duplicates a candidate on purpose)
    for name in ("wide14", "n3", "L65"):
        row = sc.BY_NAME[name]
        _, ref, _ = sc.oracle_of(row, sc.latents(row))
        e = np.sort(ref if ref.ndim == 1 else ref.sum(axis=1))
        assert e[0] < e[1] - 1e-6 * max(1.0, abs(e[0])), name
