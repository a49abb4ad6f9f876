"""The graph-walk sweep without a device (tests/walk_shape_cases.py; the device half is tests/test_gpu_walk_shapes.py).

1. walk_frames_plan, walk_score_plan and walk_time_plan are held to the C text of csrc/mg_walk.hip (its aligning list: csrc/mg_joint_plan.h
   over mg_pack.h's chain), mg_walk_score.hip and mg_walk_time.hip line by line, k_steps to mg_primitive_create.
2. FRAME_ROWS lands on both sides of every comparison of walk_frames_plan, and every row takes the routes it names.
3. The boundaries of the other two plans, as numbers: the packed / staged width, the 64 KiB opt-in and the 150 KiB refusal of the
   score kernel; the chunk count, the register / memory split of the time latents, both arms of wave_doubles and the K = 240 / 241
   refusal of the time kernel; every case of its KKg switch is a width some L + Lt gives.
4. graph_walk.assemble_walk_host -- the device sweep's reference -- is held to the oracle's control-point chain on every row of
   n_dim >= 7 that launches, under tests/test_graph_walk_host.py's WALK_TOLERANCE, with its conditioning rule (every heading's xz
   norm >= 0.1 before normalisation) and one more input condition: no step turns by more than pi - 0.05 as the oracle measures the
   turn (walk_shape_cases.oracle_walk says why).  The rows' seeds are chosen so that both hold; no row is left out.
5. TIME_ROWS and SCORE_ROWS claim every case of the KKg switch, every KK in 2 .. 16, and both sides of every comparison of their plans;
   every constrained t of every time row is at least 1e-6 from a whole number in the oracle.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import walk_shape_cases as wc
from morphablegraphs_amd import graph_walk as gw
from test_graph_walk_host import WALK_TOLERANCE, root_scale


def _source(*parts):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, *parts)).read()


def _csrc(name):
    return _source("morphablegraphs_amd", "csrc", name)


def test_restatements_match_the_source():
    walk, score, time, host = _csrc("mg_walk.hip"), _csrc("mg_walk_score.hip"), _csrc("mg_walk_time.hip"), _csrc("mg_host.hip")
    header, hostdefs = _source("include", "mg_hip.h"), _csrc("mg_hostdefs.h")
    for src, name, value in ((walk, "MG_WALK_TILE", wc.MG_WALK_TILE), (walk, "MG_WALK_BLOCK", wc.MG_WALK_BLOCK), (walk, "MG_WALK_CHAIN_BLOCK", wc.MG_WALK_CHAIN_BLOCK),
                             (time, "MG_WTIME_CHUNK", wc.MG_WTIME_CHUNK), (header, "MG_MAX_CHAIN", wc.MG_MAX_CHAIN), (header, "MG_WALK_MAX_STEPS", wc.MG_WALK_MAX_STEPS),
                             (hostdefs, "MG_MAX_KK", wc.MG_MAX_KK)):
        m = re.search(r"#define %s (\d+)\b" % name, src)
        assert m and int(m.group(1)) == value, name
    assert "#define MG_WALK_LDS_MAX (160 * 1024 - 64)" in walk and wc.MG_WALK_LDS_MAX == 163776
    assert "#define MG_WSCORE_LDS_MAX (150 * 1024)" in score and "#define MG_WTIME_LDS_MAX (150 * 1024)" in time
    assert "#define MG_WTIME_BS (MG_WTIME_CHUNK + 1)" in time
    assert wc.MG_WALK_TILE == wc._capi.MG_WALK_TILE and wc.MG_WALK_MAX_STEPS == wc._capi.MG_WALK_MAX_STEPS
    # mg_primitive_image_build (behind mg_primitive_create): the k-steps and the control-point rows
    image = _csrc("mg_primitive_image.h")
    for line in ("p->KK = (L <= 4 * MG_MAX_KK) ? (((L + 3) / 4 + 1) / 2) * 2 : 0;", "p->KKg = (Lg <= 4 * MG_MAX_KK) ? (((Lg + 3) / 4 + 1) / 2) * 2 : 0;",
                 "const int NB = d->n_basis, D = d->n_dim, L = d->n_components, K = d->n_gmm, R = NB * D;"):
        assert line in image, line
    # mg_walk_frames
    body = walk[walk.index('extern "C" int mg_walk_frames('):walk.index('extern "C" int mg_walk_frames_host(')]
    for line in ("MG_WALK_REQUIRE(n_steps >= 1 && n_steps <= MG_WALK_MAX_STEPS,", "lmax = std::max(lmax, (int)p->L);", "rmax = std::max(rmax, (int)p->R);",
                 "const bool aligned_any = n_steps > 1 || al != nullptr;", "MG_WALK_REQUIRE(D >= 3 && (!aligned_any || D >= 7),",
                 "if (al->joint == MG_ALIGN_START_POSE) {", "joint = al->joint;",
                 "if (!aligned_any) {", "a.n_link = 0;", "} else if (joint == 0 && !sk) {", "a.n_link = 1; a.link[0] = 3;",
                 "MG_WALK_REQUIRE(sk != nullptr,", "const mg_plan_failure f = mg_aligning_quaternions(sk, joint, D, quats);",
                 "MG_WALK_REQUIRE(!f, \"mg_walk_frames: the aligning chain does not fit (channel %d, n_dim %d)\", f.channel, D);",
                 "a.n_link = (int32_t)quats.size();", "std::copy(quats.begin(), quats.end(), a.link);",
                 "const size_t lds_f = ((size_t)rmax + lmax + MG_WALK_TILE * 4) * 8 + MG_WALK_TILE * 4;",
                 "const size_t lds_c = ((size_t)lmax + 5 * (3 + 4 * a.n_link) + 4) * 8 + 16;",
                 "MG_REQUIRE_AS(lds_f <= MG_WALK_LDS_MAX, MG_ERR_UNSUPPORTED,",
                 "tiles += ((lengths ? (int64_t)t_cap : (int64_t)st.T) + MG_WALK_TILE - 1) / MG_WALK_TILE;",
                 "MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_WALK_FRAMES, 160 * 1024,", "a.lmax = lmax; a.rmax = rmax;"):
        assert line in body, line
    # ... whose aligning list is mg_aligning_quaternions' (mg_joint_plan.h) over mg_joint_chain's chain (mg_pack.h)
    plan, pack = _csrc("mg_joint_plan.h"), _csrc("mg_pack.h")
    aligning = plan[plan.index("inline mg_plan_failure mg_aligning_quaternions("):]
    for line in ("f.kind = mg_joint_chain(sk->parents, sk->n_joints, node, ch, &f.joint);", "for (int j : ch) {", "if (qc < 0) continue;",
                 "if (qc + 4 > D) { f.kind = MG_PLAN_CHANNEL_OUTSIDE; return f; }",
                 "if ((int)quats.size() >= MG_MAX_CHAIN) { f.kind = MG_PLAN_TOO_LONG; f.length = MG_MAX_CHAIN + 1; return f; }", "quats.push_back(qc);"):
        assert line in aligning, line
    for line in ("for (int j = joint; j >= 0; j = parents ? parents[j] : -1) {", "out.push_back(j);", "std::reverse(out.begin(), out.end());"):
        assert line in pack, line
    assert body.index("MG_REQUIRE_AS(lds_f <= MG_WALK_LDS_MAX") < body.index("dt.upload(") < body.index("hipLaunchKernelGGL(")      # refused before anything is written
    for line in ("const int nch = 3 + 4 * a.n_link;", "for (int e = tid; e < 5 * nch; e += MG_WALK_CHAIN_BLOCK) {",
                 "const int ch = q < 3 ? q : a.link[(q - 3) >> 2] + ((q - 3) & 3);", "if (!aligned || d >= 7) return v;",
                 "const int n = nf * D, odd = (int)(((uintptr_t)dst >> 3) & 1);"):
        assert line in walk, line
    # mg_score_walk_residuals_steps
    for line in ("const bool force_valu = ctx->opt[MG_OPT_FORCE_VALU_SCORE] != 0;", "int rtmax = 0, nmax = 1, xs = 0;", "d.lat_off = s.latent_offset; d.KK = p->KK; d.L = p->L;",
                 "if (!cs || cs->n == 0) continue;", "const bool packed = cs->d_Wpack && !force_valu;", "if (packed) rtmax = std::max(rtmax, (int)cs->RT);",
                 "else xs = std::max(xs, (int)p->L + 1);", "nmax = std::max(nmax, (int)cs->n);", "const int vs = rtmax * 16 + 1;",
                 "const size_t lds = (size_t)4 * ((size_t)16 * vs + (size_t)nmax * 16 + 64 + (size_t)16 * xs) * 8;",
                 "MG_REQUIRE_AS(lds <= MG_WSCORE_LDS_MAX, MG_ERR_UNSUPPORTED,",
                 "if (lds > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_WALK_SCORE, 160 * 1024,"):
        assert line in score, line
    assert "double *d_Wpack = nullptr;  // [RT][KK][64] MFMA B fragments of W (n_components <= 64)" in _csrc("mg_internal.h")
    # mg_score_walk_time
    for line in ("MG_WTIME_REFUSE(p->K <= 0 || !p->d_gPpack || p->KKg < 2 || p->KKg > MG_MAX_KK || (p->KKg & 1) || (size_t)p->K * 16 * 16 > 60 * 1024,",
                 "d.KKg = p->KKg; d.JT = (p->Lg + 15) / 16;", "kmax = std::max(kmax, (int)p->K);", "int kmax = 1;",
                 "const int wave_doubles = std::max(16 * MG_WTIME_BS, 2 * kmax * 16);",
                 "const size_t lds = ((size_t)48 * n_steps + (size_t)16 * n_constraints + (size_t)4 * wave_doubles) * 8;",
                 "MG_WTIME_REFUSE(lds > MG_WTIME_LDS_MAX,", "if (lds > 64 * 1024) MG_HIP_CHECK(mg_lds_opt_in_once(ctx, MG_LDS_WALK_TIME, 160 * 1024,",
                 "if (Lt == 0) {   // no time model: the identity", "double gl[16];", "for (int i0 = 0; i0 < F; i0 += MG_WTIME_CHUNK) {",
                 "for (int l = 16; l < Lt; l++) e = fma(ph[l], gam[l], e);", "for (int u = wave; u < 2 * ns; u += 4) {"):
        assert line in time, line
    cases = re.findall(r"case (\d+): mg_wtime_logp<(\d+)>", time)
    assert [int(a) for a, _ in cases] == [int(b) for _, b in cases] == [2, 4, 6, 8, 10, 12, 14] and "default: mg_wtime_logp<16>" in time


def _plan(name):
    return wc.frame_plan(wc.FRAME_BY_NAME[name])


def test_the_frame_rows_land_on_both_sides_of_every_comparison():
    R = wc.FRAME_BY_NAME
    # aligned_any: one unaligned step has no links at any n_dim; D < 7 is refused as soon as anything is aligned
    for D in (3, 4, 6):
        p = _plan("single_D%d" % D)
        assert p["n_link"] == 0 and p["lds_c"] == (8 + 15 + 4) * 8 + 16 and p["chain_passes"] == 1
        for kw in (dict(first_aligned=True), dict(first_aligned=True, start_pose=True)):
            with pytest.raises(wc.Refused) as e:
                wc.walk_frames_plan([(8, 9, 33)], D, **kw)
            assert e.value.status == wc.MG_ERR_INVALID_ARGUMENT
        with pytest.raises(wc.Refused):
            wc.walk_frames_plan([(8, 9, 33), (8, 9, 33)], D)
    assert wc.walk_frames_plan([(8, 9, 33)], 7)["n_link"] == 0 and wc.walk_frames_plan([(8, 9, 33)], 7, True)["n_link"] == 1
    assert wc.walk_frames_plan([(8, 9, 33)], 2 + 1, False)["tiles_per_walk"] == 2
    # joint == 0 && !sk against the skeleton's chain; the channel list is the chain's, root first
    assert _plan("D11_2steps_previous")["link"] == [3, 7] and _plan("D7_2steps_previous")["link"] == [3] == _plan("D11_2steps_none")["link"]
    assert _plan("D11_3steps_start_pose")["link"] == [3] and _plan("D15_3steps_previous")["link"] == [3, 7]
    # 5 * (3 + 4 n_link) against the 64 lanes of the chain kernel: n_link 2 is one pass of its loop, 3 the first that takes a second
    depth = {d: _plan("chain_depth_%d" % d) for d in (1, 2, 3, 4, 7)}
    assert [depth[d]["n_link"] for d in (1, 2, 3, 4, 7)] == [1, 2, 3, 4, 7]
    assert [depth[d]["chain_passes"] for d in (1, 2, 3, 4, 7)] == [1, 1, 2, 2, 3] and 5 * 11 <= 64 < 5 * 15
    assert depth[7]["link"] == [3, 7, 11, 23, 27, 31, 35]              # Hips, Spine, Spine1, LeftShoulder, LeftArm, LeftForeArm, LeftHand
    joints, animated = wc.synthetic.make_skeleton()
    sk = wc._capi.Skeleton(joints, animated)
    assert max(sum(1 for j in sk.chain(n) if sk.quat_channel[j] >= 0) for n in animated) == 7      # the deepest chain make_skeleton gives
    # a.n_link < MG_MAX_CHAIN
    assert _plan("chain_max")["n_link"] == wc.MG_MAX_CHAIN and _plan("chain_max")["chain_passes"] == 11
    with pytest.raises(wc.Refused) as e:
        _plan("chain_one_more")
    assert e.value.status == wc.MG_ERR_INVALID_ARGUMENT == R["chain_one_more"]["expect"]
    # qc < 0: the chain Hips -> Mid -> Spine has three joints and two links
    assert _plan("chain_unanimated_joint")["link"] == [3, 7] and len(wc.skeleton_of(R["chain_unanimated_joint"])[0]) == 3
    # lmax / rmax: a step of L = 1, NB = 4 beside one of L = 64, NB = 12
    p = _plan("pitches")
    assert (p["lmax"], p["rmax"]) == (64, 12 * 11) and min(s[0] for s in R["pitches"]["shapes"]) == 1 and 4 * 11 < p["rmax"]
    assert p["tiles_per_walk"] == 1 + 2 + 1
    # lds_f <= MG_WALK_LDS_MAX: the largest block that fits, and one double more
    p = _plan("lds_largest")
    assert p["lds_f"] == wc.MG_WALK_LDS_MAX and p["rmax"] + p["lmax"] == 20328
    with pytest.raises(wc.Refused) as e:
        _plan("lds_one_more")
    assert e.value.status == wc.MG_ERR_UNSUPPORTED == R["lds_one_more"]["expect"]
    assert R["lds_one_more"]["shapes"][0][0] == R["lds_largest"]["shapes"][0][0] + 1
    # the paired store: with the walks' buffer 16-byte aligned a tile starts on double (walk * stride + offset + 32 tile) * D
    r = R["parities"]
    stride = wc.PARITY_STRIDE
    assert stride % 2 == 0 and all(max(o) + 33 <= stride for o in r["offsets"])
    seen = {(i, t, ((w * stride + r["offsets"][w][i] + 32 * t) * r["D"]) & 1) for w in range(2) for i in range(2) for t in range(2)}
    assert seen == {(i, t, b) for i in range(2) for t in range(2) for b in range(2)} and r["D"] % 2 == 1
    assert all(r["shapes"][k][1] == 33 for k in r["sequence"])         # two tiles per step, the second of one frame
    # every row that launches has a plan, and the rows' claims are what the plans say
    for r in wc.FRAME_ROWS:
        if r["expect"] is not None:
            continue
        p = wc.frame_plan(r)
        if "chain:no_links" in r["routes"]:
            assert p["n_link"] == 0
        if "chain:one_pass" in r["routes"]:
            assert p["chain_passes"] == 1 and p["n_link"] >= 1
        if "chain:more_passes" in r["routes"]:
            assert p["chain_passes"] >= 2


def test_the_frame_rows_cover_the_issues_list():
    want = {"D:%d" % D for D in (3, 4, 6, 7, 8, 11, 12, 15)} | {"mode:%s" % m for m in ("previous", "start_pose", "none")}
    want |= {"steps:2", "steps:3", "walks:1", "walks:2", "walks:5", "lat:float32", "lat:float64", "chain:no_links", "chain:one_pass", "chain:more_passes",
             "chain:max_links", "chain:unanimated_joint", "refused:chain", "refused:lds", "ref_dir:x", "ref_dir:oblique", "frames:unaligned", "frames:even_D",
             "frames:odd_D", "frames:root_is_the_whole_row", "frames:below_lmax_rmax", "frames:both_parities", "frames:lds_largest"}
    want |= {"chain:depth_%d" % d for d in (1, 2, 3, 4, 7)}
    assert wc.FRAME_ROUTES == want, sorted(wc.FRAME_ROUTES ^ want)
    # D in {7, 8, 11, 12, 15} x two and three steps x the three first-step modes: all thirty, both dtypes at every n_dim
    combos = {(r["D"], len(r["sequence"]), r["kind"]) for r in wc.FRAME_ROWS if re.match(r"D\d+_\dsteps_", r["name"])}
    assert combos == {(D, n, k) for D in (7, 8, 11, 12, 15) for n in (2, 3) for k in ("previous", "start_pose", "none")}
    for D in (7, 8, 11, 12, 15):
        assert {np.dtype(r["dtype"]).name for r in wc.FRAME_ROWS if r["name"].startswith("D%d_" % D)} == {"float32", "float64"}
    assert len({r["seed"] for r in wc.FRAME_ROWS}) == len(wc.FRAME_ROWS) and abs(np.linalg.norm(wc.OBLIQUE) - 1.0) < 1e-15
    assert min(wc.OBLIQUE) > 0.4


def test_the_other_two_plans_at_their_boundaries():
    # score: KK of every width the issue lists; 64 is the last packed width
    widths = (4, 5, 16, 17, 24, 25, 32, 33, 48, 49, 56, 57, 60, 61, 64, 65)
    assert [wc.k_steps(L) for L in widths] == [2, 2, 4, 6, 6, 8, 8, 10, 12, 14, 14, 16, 16, 16, 16, 0]
    assert {wc.k_steps(L) for L in widths} == {0} | set(range(2, 17, 2))
    p = wc.walk_score_plan([(64, [(7, 2)]), (65, [(7, None)])])
    assert [s["routes"] for s in p["steps"]] == [["packed"], ["staged"]] and (p["vs"], p["nmax"], p["xs"]) == (33, 7, 66) and not p["opt_in"]
    assert wc.walk_score_plan([(64, [(7, 2)])], force_valu=True)["steps"][0]["routes"] == ["staged"]
    # lds = 32 (16 vs + 16 nmax + 64 + 16 xs): 64 KiB between 107 and 108 constraints beside one packed row tile, 150 KiB between 279 and 280
    lds = lambda n, RT: wc.walk_score_plan([(8, [(n, RT)])])
    assert not lds(107, 1)["opt_in"] and lds(108, 1)["opt_in"] and lds(107, 1)["lds"] == 32 * (16 * 17 + 16 * 107 + 64) == wc.KB64
    assert lds(279, 1)["lds"] == wc.MG_WSCORE_LDS_MAX
    with pytest.raises(wc.Refused) as e:
        lds(280, 1)
    assert e.value.status == wc.MG_ERR_UNSUPPORTED
    # time: the chunks of 64 frames, the sixteen time latents in registers, both arms of wave_doubles, K * 256 > 60 KiB
    chunks = lambda F: wc.walk_time_plan([(F, 5, 2, 2)], 0)["steps"][0]["chunks"]
    assert [chunks(F) for F in (2, 63, 64, 65, 128, 129)] == [1, 1, 1, 2, 2, 3]
    assert [wc.walk_time_plan([(20, 5, Lt, 2)], 0)["steps"][0]["gamma_from_memory"] for Lt in (0, 1, 15, 16, 17, 20)] == [False] * 4 + [True] * 2
    assert {wc.k_steps(L + Lt) for L, Lt in ((3, 1), (9, 3), (20, 1), (25, 3), (30, 4), (40, 2), (50, 3), (60, 3))} == set(range(2, 17, 2))
    wd = lambda K: wc.walk_time_plan([(20, 5, 2, K)], 0)["wave_doubles"]
    assert [wd(K) for K in (1, 32, 33, 40)] == [1040, 1040, 1056, 1280]
    # (the mixture test K * 256 > 60 KiB would let K = 240 through, but four waves' terms and exponentials are 1024 K bytes of LDS: one
    # step fits up to K = 149 and is refused from 150 on by the LDS test, so the K = 240 / 241 pair of the mixture test cannot be met)
    assert wc.walk_time_plan([(20, 5, 2, 149)], 0)["opt_in"] is True and wc.walk_time_plan([(20, 5, 2, 149)], 0)["lds"] == 384 + 1024 * 149
    for K in (150, 240, 241):
        with pytest.raises(wc.Refused, match="LDS" if K <= 240 else "mixture"):
            wc.walk_time_plan([(20, 5, 2, K)], 0)
    assert not wc.walk_time_plan([(20, 5, 2, 63)], 0)["opt_in"] and wc.walk_time_plan([(20, 5, 2, 64)], 0)["opt_in"]
    with pytest.raises(wc.Refused):
        wc.walk_time_plan([(20, 62, 3, 2)], 0)                      # L + Lt = 65: no packed mixture
    assert [wc.walk_time_plan([(20, 5, 2, 2)] * n, 0)["units"] for n in (1, 2, 3, 4, 5, 8, 9)] == [2, 4, 6, 8, 10, 16, 18]


LAUNCHED = [r["name"] for r in wc.FRAME_ROWS if r["expect"] is None and r["D"] >= 7]


@pytest.mark.parametrize("name", LAUNCHED)
def test_assemble_walk_host_is_the_oracles_chain_on_every_row(name):
    r = wc.FRAME_BY_NAME[name]
    _, steps, S, alignment, hip_sk, skel, prev = wc.frame_case(r)
    frames, offsets, transforms = gw.assemble_walk_host(steps, S, alignment=alignment, skeleton=hip_sk)
    assert frames.shape == (r["n_walks"], sum(d["n_canonical_frames"] for d in steps), r["D"]) and not np.isnan(frames).any()
    node = r["node"] if r["kind"] == "previous" else skel[0][0][0]
    ref_dir = r["ref_dir"] if r["kind"] == "previous" else (0.0, 0.0, 1.0)
    for w in range(r["n_walks"]):
        ref, least, widest = wc.oracle_walk(steps, S[w], r["kind"], node, skel, prev, ref_dir)
        assert least >= 0.1, "a heading of row %s, walk %d is badly conditioned: %g" % (name, w, least)
        assert widest <= np.pi - 0.05, "a step of row %s, walk %d turns by %g: the oracle's half angle is the other root quaternion" % (name, w, widest)
        worst = float(np.max(np.abs(frames[w] - ref))) / root_scale(ref)
        print("row %s walk %d: disagreement %.3g of the root scale %.4g, least heading norm %.3g" % (name, w, worst, root_scale(ref), least))
        assert worst <= WALK_TOLERANCE
    assert np.allclose(transforms[..., 0] ** 2 + transforms[..., 1] ** 2, 1.0, atol=1e-12)


def test_every_row_is_held_to_the_oracle_or_to_the_back_projection():
    rest = [r for r in wc.FRAME_ROWS if r["name"] not in LAUNCHED]
    assert all(r["expect"] is not None or (r["D"] < 7 and r["kind"] == "none" and len(r["sequence"]) == 1) for r in rest)
    assert len(LAUNCHED) + len(rest) == len(wc.FRAME_ROWS) and len(rest) == 5


# ---- the time kernel's rows ---------------------------------------------------------------------------------------------------------
def test_the_time_rows_land_on_both_sides_of_every_comparison():
    S, R = wc.TIME_SHAPES, wc.TIME_ROWS
    used = {k for w, _ in R.values() for k in w}
    assert used == set(S)
    assert {S[k][0] for k in used} >= {2, 63, 64, 65, 128, 129} and {S[k][2] for k in used} >= {0, 1, 15, 16, 17, 20}
    assert {S[k][3] for k in used} >= {1, 32, 33, 40, 148, 149}
    # every case of the KKg switch is claimed by a shape some row runs
    assert {wc.k_steps(S[k][1] + S[k][2]) for k in used if k != "k149"} == set(range(2, 17, 2))
    assert {len(w) for w, _ in R.values()} >= {1, 2, 3, 4, 5, 8, 9} and {n for _, n in R.values()} >= {1, 15, 16, 17, 33}
    plans = {row: wc.time_plan(row) for row in R if row not in wc.TIME_REFUSED}
    steps = [s for p in plans.values() for s in p["steps"]]
    assert {s["chunks"] for s in steps} == {0, 1, 2, 3} and {s["gamma_from_memory"] for s in steps} == {False, True}
    assert {s["JT"] for s in steps} == {1, 2, 3, 4}
    # wave_doubles: 16 * 65 up to K = 32, 2 * K * 16 from 33 on; the 64 KiB opt-in; the LDS refusal at K = 149 beside 13 constraints (148 fills it exactly)
    assert wc.walk_time_plan([S["f128"]], 0)["wave_doubles"] == 1040 and wc.walk_time_plan([S["f129"]], 0)["wave_doubles"] == 1056
    assert wc.walk_time_plan([S["lt0"]], 0)["wave_doubles"] == 1280
    assert {p["opt_in"] for p in plans.values()} == {False, True} and plans["k148"]["opt_in"]
    with pytest.raises(wc.Refused, match="LDS") as e:
        wc.time_plan("k149")
    assert e.value.status == wc.MG_ERR_UNSUPPORTED == wc.TIME_REFUSED["k149"]
    assert {p["units"] for p in plans.values()} >= {2, 4, 6, 8, 10, 16, 18}
    # the constraints: every edge keyframe on a step where it is a frame and on one where it lies past F; from the end; two on one keyframe;
    # beyond the window; several on one step with some past F
    for row, (window, _) in R.items():
        clist = wc.time_constraints_of(window)
        F = [S[k][0] for k in window]
        inside = [(k, kf) for k, kf, _ in clist if k < len(window) and -F[k] <= kf < F[k]]
        assert len(inside) < len([c for c in clist if c[0] < len(window)]) and any(k >= len(window) for k, _, _ in clist)
        assert any(k == 10000 for k, _, _ in clist) and len(set(inside)) < len(inside)
        assert all((k, kf) in inside for k in range(len(window)) for kf in (0, F[k] - 1, -1, -F[k]))
    hit = {(S[k][0], kf) for w, _ in R.values() for k in w for kf in (62, 63, 64, 65) if kf < S[k][0]}
    assert hit >= {(63, 62), (64, 63), (65, 64), (128, 63), (128, 64), (129, 64), (129, 65), (65, 63)}


@pytest.mark.parametrize("row", [r for r in wc.TIME_IDS if r not in wc.TIME_REFUSED])
def test_no_constrained_time_is_near_a_whole_number(row):
    """int() truncates: a t within rounding of an integer could fall either way on the device.  Steps with a time model keep 1e-6;
    a step without one has t(i) = i exactly on both sides."""
    window, n, _, _, clist = wc.time_case(row)
    start, tfs, _ = wc.time_oracle_functions(row)
    assert abs(start - round(start)) >= 1e-6
    checked = 0
    for k, kf, _ in clist:
        if k >= len(window) or kf >= tfs[k].shape[1]:
            continue
        t = tfs[k][:, kf]
        if wc.TIME_SHAPES[window[k]][2] == 0:
            assert np.array_equal(t, np.full(n, float(kf % tfs[k].shape[1])))
        else:
            assert np.all(np.abs(t - np.round(t)) >= 1e-6), (row, k, kf, t)
        checked += 1
    assert checked >= 4 and all(np.isfinite(tf).all() for tf in tfs)


# ---- the score kernel's rows --------------------------------------------------------------------------------------------------------
def test_the_score_rows_claim_every_k_step_count_and_both_routes():
    R = wc.SCORE_ROWS
    launched = {L for row, (w, _, _, _, what) in R.items() if "refused" not in what for L in w}
    assert launched == set(wc.SCORE_WIDTHS) and {wc.k_steps(L) for L in launched} == {0} | set(range(2, 17, 2))
    assert all(2 <= len(w) <= 3 for w, _, _, _, _ in R.values())
    assert {c for _, c, _, _, _ in R.values()} >= {1, 2, 15, 16, 17} and {n for _, _, n, _, _ in R.values()} >= {1, 16, 17, 64, 65}
    assert {np.dtype(d).name for _, _, _, d, _ in R.values()} == {"float32", "float64"}
    assert {x for _, _, _, _, what in R.values() for x in what} == {"errors_only", "wide_ld", "descending", "force_valu", "deep", "refused"}
    # packed beside staged in one walk, on both sides of L = 64 / 65
    assert R["edge"][0] == (64, 65) and wc.k_steps(64) == 16 and wc.k_steps(65) == 0
    # the refused walk: whatever the row tiles of its packed step (at least one), the staged tile of L = 280 leaves no room
    L = wc.SCORE_REFUSED_L
    with pytest.raises(wc.Refused) as e:
        wc.walk_score_plan([(L, [(5, None)]), (4, [(5, 1)])])
    assert e.value.status == wc.MG_ERR_UNSUPPORTED and wc.walk_score_plan([(L, [(5, None)])])["lds"] <= wc.MG_WSCORE_LDS_MAX
    # the deep row: two seven-link chains are at least 2 * 31 channel rows (RT >= 4); beside the staged L = 65 tile that is past 64 KiB
    # from RT = 3 on and below 150 KiB up to RT = 13
    assert wc.walk_score_plan([(65, [(6, None)]), (33, [(6, 4)])])["opt_in"] and wc.walk_score_plan([(65, [(6, None)]), (33, [(6, 13)])])["opt_in"]
    assert not wc.walk_score_plan([(65, [(6, None)]), (33, [(6, 2)])])["opt_in"]
