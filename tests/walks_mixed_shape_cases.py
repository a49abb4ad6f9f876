"""The mixed-population walk kernels' host decisions restated, and the table of shapes on both sides of every one of them.

Shared by tests/test_walks_mixed_shapes_host.py (no device: the restatements against the C text, the tables against the restatements,
the NumPy statements against the oracle and the 50-digit twin on every row) and tests/test_gpu_walks_mixed_shapes.py (the same rows on
the device, with a ledger of the routes they took).

walks_frames_plan restates mg_walks_frames_launch, walks_sample_plan mg_walks_sample_latents and walks_time_plan mg_walks_time_launch
(all csrc/mg_walks_mixed.hip).  A row of MIXED_FRAME_ROWS is one population: its nodes, its walks (named, not drawn), its alignment,
its latent dtype, its frame offsets and, for the WARPED = true kernels, its hand-made time rows.  DERIVED names the routes a row may
only claim when frame_routes derives them from the plan's own numbers.  The constants, the skeletons, the start pose and the oracle's
chain are tests/walk_shape_cases.py's.
"""
import functools

import numpy as np

import random_walk_cases as rc
import timewarp_cases as tc
import walk_shape_cases as wc
from morphablegraphs_amd import _capi, synthetic
from morphablegraphs_amd.candidate_scoring import alignment_from_start_pose
from morphablegraphs_amd.graph_walk import _basis_rows, _untimed_grid          # NumPy only: the basis row of a time, the canonical grid
from oracle import mg_oracle as orc

MG_OK = _capi.MG_OK
INVALID, UNSUPPORTED = wc.MG_ERR_INVALID_ARGUMENT, wc.MG_ERR_UNSUPPORTED
Refused = wc.Refused

# ---- constants of csrc/mg_walks_mixed.hip and csrc/mg_timewarp_device.h (pinned by test_the_constants_are_the_sources) --------------
MG_WALKS_TILE = 32
MG_WALKS_BLOCK = 256
MG_WALKS_CHAIN_BLOCK = 64
MG_WALKS_SAMPLE_BLOCK = 64
MG_WALKS_LDS_MAX = 160 * 1024 - 64
MG_WALKS_SAMPLE_LDS_MAX = 150 * 1024
MG_TW_BLOCK = 64
MG_TW_MAX_F = 2048
MG_TW_SMOOTH_W = 15
MG_TW_SMOOTH_LDS = (MG_TW_BLOCK + 2 * 7) + 2 * MG_TW_SMOOTH_W
KB64 = wc.KB64


# ---- what the three launches share: mg_walks_check_tables --------------------------------------------------------------------------
def _check_tables(n_nodes, walks):
    """occurs[k]; the walks are lists of node indices, so n_steps[w] = len(walks[w]) and s_max their longest (1 for no walk)."""
    if n_nodes < 1:
        raise Refused(INVALID, "no nodes")
    occurs = [False] * n_nodes
    for seq in walks:
        if len(seq) < 1:
            raise Refused(INVALID, "a walk without steps")
        for k in seq:
            if not 0 <= k < n_nodes:
                raise Refused(INVALID, "names node %d of %d" % (k, n_nodes))
            occurs[k] = True
    return occurs


def s_max_of(walks):
    return max([len(seq) for seq in walks] + [1])


@functools.lru_cache(maxsize=None)
def _canonical_i0(F, NB):
    """The first taps of the canonical grid numpy.linspace(0, F, F) of a primitive of F canonical frames and NB basis functions."""
    return _basis_rows(synthetic.cubic_b_spline_knots(NB, F), _untimed_grid(F))[0]


# ---- mg_walks_frames_launch ---------------------------------------------------------------------------------------------------------
def walks_frames_plan(nodes, D, walks, first_aligned=False, start_pose=False, joint=0, skeleton=None, lengths=None, frame_offset=None, walk_stride=None,
                      times=None, t_cap=None, ld=None):
    """nodes: (L, F, NB) per node; walks: a list of node indices per walk; first_aligned: an alignment record is given; start_pose: it
    is a start pose; joint: the record's node; skeleton: None or (parents, quat_channel); lengths / times: None (the canonical grids)
    or lengths[w][i] and times[w][i], the samples of every step's time row (mg_walks_frames_at); frame_offset: None (back to back) or
    frame_offset[w][i]; walk_stride: None (the longest walk's end).  Raises Refused with the status the library answers."""
    occurs = _check_tables(len(nodes), walks)
    warped = lengths is not None
    if warped:
        t_cap = max([lengths[w][i] for w, seq in enumerate(walks) for i in range(len(seq))] + [1]) if t_cap is None else t_cap
        if t_cap < 1 or (walks and (times is None or frame_offset is None)):
            raise Refused(INVALID, "times, lengths and frame offsets are required")
    lmax, rmax = 0, 0
    for k, (L, F, NB) in enumerate(nodes):
        if occurs[k] and ld is not None and L > ld:
            raise Refused(INVALID, "ld")
        lmax, rmax = max(lmax, L), max(rmax, NB * D)
    aligned_any = first_aligned or any(len(seq) > 1 for seq in walks)
    if not (D >= 3 and (not aligned_any or D >= 7)):
        raise Refused(INVALID, "no root channels to align")
    if not first_aligned or start_pose:
        joint = 0
    link = []
    if not aligned_any:
        pass
    elif joint == 0 and skeleton is None:
        link = [3]
    else:
        if skeleton is None:
            raise Refused(INVALID, "a skeleton is needed")
        parents, quat_channel = skeleton
        chain, j = [], joint
        while j >= 0:
            chain.insert(0, j)
            j = int(parents[j])
        for j in chain:
            qc = int(quat_channel[j])
            if qc < 0:
                continue
            if not (qc + 4 <= D and len(link) < wc.MG_MAX_CHAIN):
                raise Refused(INVALID, "the aligning chain does not fit")
            link.append(qc)
    n_link = len(link)
    # offsets and tiles: every step inside its walk's rows, no two steps on the same row
    offs, step_tile, walk_tile, ends, tiles = [], [], [0], [], 0
    for w, seq in enumerate(walks):
        nxt, walk_tiles, spans, o_w, t_w = 0, 0, [], [], []
        for i, k in enumerate(seq):
            n = lengths[w][i] if warped else nodes[k][1]
            if warped and not 1 <= n <= t_cap:
                raise Refused(INVALID, "samples")
            off = frame_offset[w][i] if frame_offset is not None else nxt
            if off < 0:
                raise Refused(INVALID, "starts at a negative row")
            o_w.append(off)
            t_w.append(walk_tiles)
            spans.append((off, n))
            nxt = off + n
            walk_tiles += (n + MG_WALKS_TILE - 1) // MG_WALKS_TILE
        end = 0
        for off, n in sorted(spans):
            if off < end:
                raise Refused(INVALID, "steps overlap")
            end = off + n
        ends.append(end)
        tiles += walk_tiles
        offs.append(o_w)
        step_tile.append(t_w)
        walk_tile.append(tiles)
    walk_stride = max(ends + [1]) if walk_stride is None else walk_stride
    if walk_stride < 1 or any(end > walk_stride for end in ends):
        raise Refused(INVALID, "walk_stride")
    nch = 3 + 4 * n_link
    plan = dict(n_link=n_link, link=link, nch=nch, lmax=lmax, rmax=rmax, tiles=tiles, walk_tile=walk_tile, step_tile=step_tile, offsets=offs,
                walk_stride=walk_stride, s_max=s_max_of(walks), launched=len(walks) > 0, chain_trips=(5 * nch + MG_WALKS_CHAIN_BLOCK - 1) // MG_WALKS_CHAIN_BLOCK,
                occurs=occurs, t_cap=t_cap)
    if not walks:
        return plan
    lds_f = (rmax + lmax + MG_WALKS_TILE * 4) * 8 + MG_WALKS_TILE * 4
    lds_c = (lmax + 5 * nch + 4) * 8 + 16
    if not lds_f <= MG_WALKS_LDS_MAX:
        raise Refused(UNSUPPORTED, "do not fit LDS")
    plan.update(lds_f=lds_f, lds_c=lds_c, opt_in=True)
    # what every workgroup of the frames kernel meets: the window of control-point rows and the pairs of its store loop (for a
    # destination on an even and on an odd double; `parity` is the tile's own when the frames buffer is 16-byte aligned)
    per_tile = []
    for w, seq in enumerate(walks):
        for i, k in enumerate(seq):
            L, F, NB = nodes[k]
            if warped:
                n = lengths[w][i]
                i0 = _basis_rows(synthetic.cubic_b_spline_knots(NB, F), np.asarray(times[w][i], dtype=np.float64)[:n])[0]
            else:
                n, i0 = F, _canonical_i0(F, NB)
            for f0 in range(0, n, MG_WALKS_TILE):
                nf = min(MG_WALKS_TILE, n - f0)
                imin, imax = int(i0[f0:f0 + nf].min()), int(i0[f0:f0 + nf].max())
                doubles = nf * D
                per_tile.append(dict(walk=w, step=i, node=k, f0=f0, nf=nf, rows=(imax + 4 - imin) * D, npairs=((doubles + 1) >> 1, (doubles + 2) >> 1),
                                     parity=((w * walk_stride + offs[w][i] + f0) * D) & 1, whole_spline=(imax + 4 - imin) == NB, L=L))
    assert len(per_tile) == tiles
    plan["per_tile"] = per_tile
    return plan


# ---- mg_walks_sample_latents --------------------------------------------------------------------------------------------------------
def walks_sample_plan(mixtures, walks, ld):
    """mixtures: (K, Lg) per node."""
    occurs = _check_tables(len(mixtures), walks)
    if ld < 1:
        raise Refused(INVALID, "bad arguments")
    lgmax = 0
    for k, (K, Lg) in enumerate(mixtures):
        if K <= 0:
            raise Refused(INVALID, "no mixture")
        if occurs[k] and Lg > ld:
            raise Refused(INVALID, "ld")
        lgmax = max(lgmax, Lg)
    rows = len(walks) * s_max_of(walks)
    if not walks:
        return dict(launched=False, rows=0, lgmax=lgmax)
    lds = MG_WALKS_SAMPLE_BLOCK * (lgmax + 1) * 8
    if not lds <= MG_WALKS_SAMPLE_LDS_MAX:
        raise Refused(UNSUPPORTED, "does not fit LDS")
    return dict(launched=True, rows=rows, lgmax=lgmax, lds=lds, opt_in=lds > KB64, grid=(rows + MG_WALKS_SAMPLE_BLOCK - 1) // MG_WALKS_SAMPLE_BLOCK)


def largest_sample_width():
    """The widest mixture whose normals fit MG_WALKS_SAMPLE_LDS_MAX: 64 lanes of Lg + 1 doubles."""
    return MG_WALKS_SAMPLE_LDS_MAX // (MG_WALKS_SAMPLE_BLOCK * 8) - 1


# ---- mg_walks_time_launch -----------------------------------------------------------------------------------------------------------
def walks_time_plan(nodes, walks, ld, speed, t_cap, smooth=None):
    """nodes: (F, L, Lt) per node; smooth: None (mg_walks_time_functions) or a flag per node (mg_walks_time_functions_smoothed)."""
    occurs = _check_tables(len(nodes), walks)
    if ld < 1 or t_cap < 1 or not (speed > 0.0 and np.isfinite(speed)):
        raise Refused(INVALID, "bad arguments")
    inv_speed, fmax, counts = 1.0 / speed, 0, [0] * len(nodes)
    for k, (F, L, Lt) in enumerate(nodes):
        if not occurs[k]:
            continue
        if L + Lt > ld:
            raise Refused(INVALID, "ld")
        if Lt > 0:
            if not 4 <= F <= MG_TW_MAX_F:
                raise Refused(UNSUPPORTED, "canonical frames")
            fmax = max(fmax, F)
        else:
            countf = F * inv_speed
            if not countf >= 1.0:
                raise Refused(INVALID, "no sample at this speed")
            if not countf <= 16777216.0:
                raise Refused(UNSUPPORTED, "samples")
            counts[k] = int(countf)
    rows = len(walks) * s_max_of(walks)
    if not walks:
        return dict(launched=False, grid=0, counts=counts)
    lds = (4 * fmax + (MG_TW_SMOOTH_LDS if smooth is not None else 0)) * 8
    return dict(launched=True, grid=rows, lds=lds, opt_in=True, fmax=fmax, counts=counts)


# ---- the frames kernels' table ------------------------------------------------------------------------------------------------------
SMALL = [(5, 12, 7), (8, 33, 9), (3, 20, 6)]            # (n_components, n_canonical_frames, n_basis): walk_shape_cases.SMALL
THREE = [[1], [0, 1], [2, 0, 1]]                        # walks of one, two and three steps
FIVE = [[1], [0, 1], [2, 0, 1], [1, 1], [0]]
PITCHES = [(1, 12, 4), (64, 40, 12), (257, 12, 6)]      # far below lmax / rmax; the node that sets rmax; the node that sets lmax
WIDE = [(65, 33, 9), (8, 33, 9), (257, 12, 5)]          # n_dim 39: L on both sides of the chain kernel's 64 and the frames kernel's 256 lanes
EDGES = [(8, 33, 9), (5, 64, 10), (3, 32, 6)]           # last tiles of one frame and of 32
GUARD_ROWS = 3
# the routes a row may claim only from its plan's numbers (frame_routes)
DERIVED = {"frames:cp_second_trip", "frames:store_second_trip", "frames:latents_second_trip", "chain:entries_second_trip", "chain:latents_second_trip",
           "frames:both_parities", "frames:even_D", "frames:below_lmax_rmax", "frames:last_tile_one_frame", "frames:last_tile_32_frames",
           "frames:lds_largest", "tables:padded_behind_the_ends", "warped:whole_spline_tile", "chain:no_links", "chain:max_links"}
WARPED_LENGTHS = (31, 1, 32, 2, 33, 64, 65)


def _row(name, D, routes, nodes=SMALL, walks=THREE, kind="previous", node="Hips", ref_dir=(0.0, 0.0, 1.0), skel=None, dtype=np.float64, offsets=None,
         expect=None, seed=None, warped=False, bound=None):
    return dict(name=name, D=D, routes=set(routes), shapes=list(nodes), walks=[list(s) for s in walks], kind=kind, node=node, ref_dir=tuple(ref_dir),
                skel=skel if skel is not None else ("humanoid", max(1, (D - 3) // 4)), dtype=dtype, offsets=offsets, expect=expect, seed=seed, warped=warped,
                bound=bound, n_walks=len(walks))


def _gapped(walks, nodes, first=3):
    """Frame offsets with gaps; odd walks hold their last step first."""
    out = []
    for w, seq in enumerate(walks):
        at, row = [0] * len(seq), first
        for i in (reversed(range(len(seq))) if w % 2 else range(len(seq))):
            at[i] = row
            row += nodes[seq[i]][1] + 1 + i
        out.append(at)
    return out


def _frame_rows():
    rows = []
    for D in (3, 4, 6):                  # one-step walks over two nodes, nothing aligned: the chain kernel reads the root translation alone
        rows.append(_row("single_D%d" % D, D, {"D:%d" % D, "chain:no_links", "frames:unaligned"}, walks=[[0], [1], [1], [0]], kind="none"))
    rows.append(_row("D6_one_two_step_walk", 6, {"refused:D_below_7"}, walks=[[0], [1], [1, 0], [0]], kind="none", expect=INVALID))
    dtypes, i = (np.float64, np.float32), 0
    for D in (7, 8, 11, 12, 15):
        for kind in ("none", "previous", "start_pose"):
            node = "Spine" if (kind == "previous" and D >= 11) else "Hips"
            walks = FIVE if i % 2 else THREE
            routes = {"D:%d" % D, "mode:%s" % kind, "steps:1_2_3", "walks:%d" % len(walks), "lat:%s" % np.dtype(dtypes[i % 2]).name}
            if D % 2 == 0:
                routes.add("frames:even_D")
            if D == 7:
                routes.add("frames:root_is_the_whole_row")
            rows.append(_row("D%d_%s" % (D, kind), D, routes, walks=walks, kind=kind, node=node, dtype=dtypes[i % 2]))
            i += 1
    D = 3 + 4 * wc.N_DEEP
    for node, depth in (("Hips", 1), ("Spine", 2), ("Spine1", 3), ("Neck", 4), ("LeftHand", 7)):
        routes = {"chain:depth_%d" % depth, "frames:cp_second_trip", "frames:store_second_trip"} | ({"chain:entries_second_trip"} if depth >= 3 else set())
        rows.append(_row("chain_depth_%d" % depth, D, routes, node=node, skel=("humanoid", wc.N_DEEP)))
    rows.append(_row("chain_max", 3 + 4 * wc.MG_MAX_CHAIN, {"chain:max_links", "chain:entries_second_trip"}, walks=[[0, 1], [1]], node="j%d" % (wc.MG_MAX_CHAIN - 1),
                     skel=("line", wc.MG_MAX_CHAIN)))
    rows.append(_row("chain_one_more", 3 + 4 * (wc.MG_MAX_CHAIN + 1), {"refused:chain"}, walks=[[0, 1], [1]], node="j%d" % wc.MG_MAX_CHAIN,
                     skel=("line", wc.MG_MAX_CHAIN + 1), expect=INVALID))
    rows.append(_row("chain_unanimated_joint", 11, {"chain:unanimated_joint"}, node="Spine", skel=("gap",)))
    rows.append(_row("ref_dir_x", 11, {"ref_dir:x"}, node="Spine", ref_dir=(1.0, 0.0, 0.0)))
    rows.append(_row("ref_dir_oblique", 11, {"ref_dir:oblique"}, node="Spine", ref_dir=wc.OBLIQUE, dtype=np.float32))
    # the second trips, at the smallest sizes that reach them: nine control-point rows of 39 channels, 32 frames of 39 channels, L = 65 / 257
    rows.append(_row("second_trips", D, {"frames:cp_second_trip", "frames:store_second_trip", "frames:latents_second_trip", "chain:latents_second_trip",
                                         "chain:entries_second_trip"}, nodes=WIDE, walks=[[0, 1], [2, 0], [1], [1, 2, 0]], node="Spine1", skel=("humanoid", wc.N_DEEP)))
    # the small node's steps before, between and after the large ones'
    rows.append(_row("pitches", 11, {"frames:below_lmax_rmax", "frames:latents_second_trip", "chain:latents_second_trip"}, nodes=PITCHES,
                     walks=[[0, 1, 0, 2], [1, 0, 2, 0], [0], [2, 1]], kind="start_pose"))
    par_walks = [[0, 1], [1, 0], [1]]
    rows.append(_row("parities", 11, {"frames:both_parities", "frames:last_tile_one_frame", "offsets:given"}, nodes=[(8, 33, 9), (5, 33, 7)], walks=par_walks,
                     offsets=[[0, 34], [1, 35], [2]]))
    rows.append(_row("offsets_with_gaps", 11, {"offsets:gaps_out_of_order", "offsets:given"}, walks=FIVE, offsets=_gapped(FIVE, SMALL), dtype=np.float32))
    rows.append(_row("tile_edges", 12, {"frames:last_tile_one_frame", "frames:last_tile_32_frames", "frames:even_D"}, nodes=EDGES, walks=[[0, 1], [2], [1, 2, 0]],
                     kind="start_pose"))
    rows.append(_row("lds_largest", wc.LDS_D, {"frames:lds_largest"}, nodes=[(wc.LDS_L, wc.LDS_F, wc.LDS_NB), (3, 12, 4)], walks=[[0], [1]], kind="start_pose"))
    rows.append(_row("lds_one_more", wc.LDS_D, {"refused:lds"}, nodes=[(wc.LDS_L + 1, wc.LDS_F, wc.LDS_NB), (3, 12, 4)], walks=[[0], [1]], kind="start_pose",
                     expect=UNSUPPORTED))
    rows.append(_row("population_1", 11, {"walks:1"}, walks=[[2, 0, 1]]))
    rows.append(_row("population_2", 11, {"walks:2"}, walks=[[1], [0, 2]], kind="start_pose", dtype=np.float32))
    rows.append(_row("population_64", 11, {"walks:64"}, walks=[[0], [1, 0], [2], [0, 1, 2]] * 16, kind="start_pose"))
    # one walk of four steps among 64 of one: node_of is padded with -1 behind 64 ends
    rows.append(_row("population_65", 11, {"walks:65", "tables:padded_behind_the_ends", "steps:4"}, walks=[[w % 3] for w in range(17)] + [[0, 1, 2, 1]] + [[w % 3] for w in range(47)]))
    rows.append(_row("no_walks", 11, {"walks:0"}, walks=[], kind="none"))
    # the WARPED = true kernels on a subset, every step at a hand-made time row (warped_times)
    for base in ("second_trips", "D12_start_pose", "D8_previous", "chain_depth_3", "pitches", "D11_none"):
        b = [r for r in rows if r["name"] == base][0]
        keep = {r for r in b["routes"] if r in DERIVED and r != "frames:last_tile_one_frame"} | {"warped:%s" % base}
        rows.append(dict(b, name="warped_" + base, warped=True, seed=None,
                         routes=keep | {"warped:lengths", "warped:on_knots", "warped:repeated_times", "warped:whole_spline_tile"}))
    for k, r in enumerate(rows):
        if r["seed"] is None:
            r["seed"] = 11000 + 20 * k          # the row's primitives take seed, seed + 1, ...; its latents seed + 10; its previous frame seed + 11
        r["seed"] = SEEDS.get(r["name"], r["seed"])
    return rows


# the first of seed + 1000, seed + 2000, ... at which the row meets the CPU half's two input conditions (every other row meets them as it is)
SEEDS = {"D12_none": 12260, "chain_depth_4": 12440, "chain_depth_7": 12460, "second_trips": 14580, "warped_second_trips": 16820}


MIXED_FRAME_ROWS = _frame_rows()
FRAME_IDS = [r["name"] for r in MIXED_FRAME_ROWS]
FRAME_BY_NAME = {r["name"]: r for r in MIXED_FRAME_ROWS}


def frame_models(row):
    """The row's primitives (JSON dicts), each from its own seed."""
    return [synthetic.make_primitive(seed=row["seed"] + i, n_components=L, n_frames=F, n_basis=NB, n_dim=row["D"], n_gmm=1, name="%s_%d" % (row["name"], i))
            for i, (L, F, NB) in enumerate(row["shapes"])]


def frame_ld(row):
    return max(L for L, _, _ in row["shapes"]) + 2         # wider than the widest node's latents


def warped_times(row):
    """(lengths[w][i], times[w][i]) of a warped row: the lengths of WARPED_LENGTHS in turn over the steps; every row of more than two
    samples runs from 0 to F - 1 with one sample exactly on an interior knot and one time repeated, a row of two is the two ends, a row
    of one an interior knot; the population's first row of 31 or 32 samples descends, so that its one tile spans the whole spline."""
    lengths, times, k, descended = [], [], 0, False
    for seq in row["walks"]:
        l_w, t_w = [], []
        for node in seq:
            _, F, NB = row["shapes"][node]
            T = WARPED_LENGTHS[k % len(WARPED_LENGTHS)]
            k += 1
            knot = float(synthetic.cubic_b_spline_knots(NB, F)[4 if NB > 4 else 3])
            if T == 1:
                t = np.array([knot])
            elif T == 2:
                t = np.array([0.0, F - 1.0])
            else:
                t = np.linspace(0.0, F - 1.0, T)
                t[3], t[6] = knot, t[5]
                if T in (31, 32) and not descended:
                    t, descended = np.sort(t)[::-1].copy(), True
            l_w.append(T)
            t_w.append(t)
        lengths.append(l_w)
        times.append(t_w)
    return lengths, times


def frame_tables(row):
    """(node_of, n_steps) as the library takes them; one column of -1 for a population of no walks."""
    if not row["walks"]:
        return np.zeros((0, 1), dtype=np.int32), np.zeros(0, dtype=np.int32)
    return rc.tables(row["walks"])


def frame_layout(row):
    """(lengths or None, times or None, frame offsets or None as lists, walk_stride): where every step of the row lies."""
    lengths, times = warped_times(row) if row["warped"] else (None, None)
    n_of = (lambda w, i, k: lengths[w][i]) if row["warped"] else (lambda w, i, k: row["shapes"][k][1])
    offsets = row["offsets"]
    if row["warped"]:                                     # given offsets, back to back with a gap of w + i rows before every step
        offsets = []
        for w, seq in enumerate(row["walks"]):
            at, o_w = 0, []
            for i, k in enumerate(seq):
                at += w + i
                o_w.append(at)
                at += lengths[w][i]
            offsets.append(o_w)
    if offsets is None:
        ends = [sum(n_of(w, i, k) for i, k in enumerate(seq)) for w, seq in enumerate(row["walks"])]
    else:
        ends = [max(offsets[w][i] + n_of(w, i, k) for i, k in enumerate(seq)) for w, seq in enumerate(row["walks"])]
    stride = max(ends + [1]) + GUARD_ROWS
    return lengths, times, offsets, stride + (stride & 1 if row["name"] == "parities" else 0)


def frame_plan(row):
    """walks_frames_plan of the row as the sweep calls the library."""
    joints, animated = wc.skeleton_of(row)
    previous = row["kind"] == "previous"
    sk = None
    if previous and row["node"] != joints[0][0]:
        s = _capi.Skeleton(joints, animated)
        sk = (s.parents, s.quat_channel)
    names = [j[0] for j in joints]
    lengths, times, offsets, stride = frame_layout(row)
    return walks_frames_plan(row["shapes"], row["D"], row["walks"], row["kind"] != "none", row["kind"] == "start_pose", names.index(row["node"]) if previous else 0, sk,
                             lengths, offsets, stride, times=times, ld=frame_ld(row))


def frame_routes(row, plan):
    """The routes of DERIVED the plan's numbers give this row."""
    out, tiles = set(), plan.get("per_tile", [])
    used = [row["shapes"][k] for k in range(len(row["shapes"])) if plan["occurs"][k]]
    if any(t["rows"] > MG_WALKS_BLOCK for t in tiles):
        out.add("frames:cp_second_trip")
    if any(t["npairs"][t["parity"]] > MG_WALKS_BLOCK for t in tiles):
        out.add("frames:store_second_trip")
    if any(L > MG_WALKS_BLOCK for L, _, _ in used):
        out.add("frames:latents_second_trip")
    if plan["launched"] and 5 * plan["nch"] > MG_WALKS_CHAIN_BLOCK:
        out.add("chain:entries_second_trip")
    if plan["n_link"] >= 1 and any(L > MG_WALKS_CHAIN_BLOCK for L, _, _ in used):
        out.add("chain:latents_second_trip")
    if row["D"] % 2 == 1 and {t["parity"] for t in tiles} == {0, 1} and {(t["parity"], t["nf"] & 1) for t in tiles} >= {(0, 1), (1, 1), (0, 0), (1, 0)}:
        out.add("frames:both_parities")
    if row["D"] % 2 == 0 and tiles and all(t["parity"] == 0 for t in tiles):
        out.add("frames:even_D")
    if any(L < plan["lmax"] // 8 and NB * row["D"] < plan["rmax"] // 2 for L, _, NB in used) and any(L == plan["lmax"] for L, _, _ in used) \
            and any(NB * row["D"] == plan["rmax"] for _, _, NB in used):
        out.add("frames:below_lmax_rmax")
    last = {(t["walk"], t["step"]): t["nf"] for t in tiles}      # (the last tile of every step overwrites the ones before it)
    if 1 in last.values():
        out.add("frames:last_tile_one_frame")
    if MG_WALKS_TILE in last.values():
        out.add("frames:last_tile_32_frames")
    if plan.get("lds_f") == MG_WALKS_LDS_MAX:
        out.add("frames:lds_largest")
    if plan["launched"] and sum(len(seq) == plan["s_max"] for seq in row["walks"]) == 1 and len(row["walks"]) > 1:
        out.add("tables:padded_behind_the_ends")
    if row["warped"] and any(t["whole_spline"] and t["nf"] > 1 for t in tiles):
        out.add("warped:whole_spline_tile")
    if plan["launched"] and plan["n_link"] == 0:
        out.add("chain:no_links")
    if plan["n_link"] == wc.MG_MAX_CHAIN:
        out.add("chain:max_links")
    return out


def frame_case(row, models=None):
    """(models, P float64 (n_walks, s_max, ld) holding the values the row's dtype holds, alignment record or None, _capi.Skeleton or
    None, (joints, animated), previous frame or None).  Every entry of P is drawn: a kernel that reads past a step's own columns, or a
    step the walk does not have, meets numbers."""
    models = frame_models(row) if models is None else models
    joints, animated = wc.skeleton_of(row)
    node_of, _ = frame_tables(row)
    P = 0.7 * np.random.default_rng(row["seed"] + 10).standard_normal(node_of.shape + (frame_ld(row),))
    if row["dtype"] == np.float32:
        P = P.astype(np.float32).astype(np.float64)
    prev, alignment, hip_sk = None, None, None
    if row["D"] >= 7:
        hip_sk = _capi.Skeleton(joints, animated)
    if row["kind"] == "previous":
        prng = np.random.default_rng(row["seed"] + 11)
        prev = orc.OraclePrimitive(models[-1]).back_project_frames(prng.standard_normal(row["shapes"][-1][0]))[-1].copy()
        prev[0] += 120.0
        prev[2] -= 40.0
        alignment = hip_sk.alignment_to(prev, row["node"], row["ref_dir"])
    elif row["kind"] == "start_pose":
        alignment = alignment_from_start_pose(wc.START_POSE)
    needs_sk = row["kind"] == "previous" and row["node"] != joints[0][0]
    return models, P, alignment, (hip_sk if needs_sk else None), (joints, animated), prev


def walk_latents(row, P, w):
    """Walk w's latents packed into one row, as the one-sequence call takes them."""
    return np.concatenate([P[w, i, :row["shapes"][k][0]] for i, k in enumerate(row["walks"][w])])


def oracle_walk(steps, row_latents, kind, node, skel, prev, ref_dir=(0.0, 0.0, 1.0), times=None):
    """walk_shape_cases.oracle_walk; with times (one row per step) the same chain with orc.spline_frames at the row's own times, the exit
    pose at the row's last entry: (frames, smallest xz norm of any heading before normalisation, widest turn)."""
    if times is None:
        return wc.oracle_walk(steps, row_latents, kind, node, skel, prev, ref_dir)
    joints, animated = skel
    parts, off, least, widest = [], 0, np.inf, 0.0
    ref = np.asarray(ref_dir, dtype=np.float64)

    def xz_norm(pose):
        p = orc.joint_global_orientation(pose, joints, animated, node) @ ref
        return float(np.hypot(p[0], p[2]))
    if prev is not None:
        least = xz_norm(prev)
    for i, data in enumerate(steps):
        op = orc.OraclePrimitive(data)
        coeffs = op.back_project_spatial_coeffs(row_latents[off:off + op.n_components])
        off += op.n_components
        if prev is not None or kind == "previous":
            least = min(least, xz_norm(coeffs[0]))
        if prev is not None:
            ha, hb = (orc.node_heading(p, joints, animated, node, ref_dir) for p in (prev, coeffs[0]))
            widest = max(widest, abs(np.arctan2(hb[1], hb[0]) - np.arctan2(ha[1], ha[0])))
            coeffs = orc.align_coeffs_to_previous_frame(coeffs, prev, joints, animated, node, ref_dir)
        elif i == 0 and kind == "start_pose":
            coeffs = orc.align_coeffs_to_start_pose(coeffs, dict(wc.START_POSE))
        fr = orc.spline_frames(op.knots, coeffs, np.asarray(times[i], dtype=np.float64))
        prev = fr[-1]
        if i + 1 < len(steps):
            least = min(least, xz_norm(prev))
        parts.append(fr)
    return np.concatenate(parts), least, widest


def place_walks(frames, offsets, row, layout_offsets, stride):
    """assemble_walks_mixed_host's walks moved to the row's frame offsets over a NaN sentinel: (n_walks, stride, D)."""
    out = np.full((len(frames), stride, row["D"]), np.nan)
    for w, fr in enumerate(frames):
        if layout_offsets is None:
            out[w, :len(fr)] = fr
            continue
        for i, at in enumerate(layout_offsets[w]):
            a, b = int(offsets[w][i]), int(offsets[w][i + 1])
            out[w, at:at + (b - a)] = fr[a:b]
    return out


# ---- the time kernel's table --------------------------------------------------------------------------------------------------------
TIME_LD = tc.N_SPATIAL + max(tc.TIME_COMPONENTS) + 3     # wider than L + Lt of every node
UNTIMED = {"u2": 2, "u4": 4, "u24": 24, "u64": 64, "u65": 65}      # nodes without a time model: name -> canonical frames


def _time_row(name, speed, nodes, walks, dtype=np.float64, short=False, smooth=(), expect=None, sized=None):
    return dict(name=name, speed=speed, nodes=list(nodes), walks=[list(s) for s in walks], dtype=dtype, short=short, smooth=tuple(smooth), expect=expect,
                sized=sized, ld=TIME_LD)


def _time_rows():
    K = lambda F: [(F, Lt) for Lt in tc.TIME_COMPONENTS]
    small = K(4) + K(5) + K(6) + ["u64", "u65"]          # at speed 1 the untimed nodes have 64 and 65 samples
    small_walks = [[0, 9, 1], [2], [3, 4], [10, 5, 6], [7, 8, 9], [10], [1, 0]]
    mid = K(63) + K(64) + K(65) + ["u2", "u4"]           # at speed 1.6: int(2 * 0.625) = 1 and int(4 * 0.625) = 2 samples
    mid_walks = [[0, 1, 9], [10, 2], [3], [4, 10, 5], [6, 7], [8, 9, 0]]
    big = K(129) + [(6, 2), "u24"]                       # at speed 0.37: int(24 * (1 / 0.37)) = 64 samples
    big_walks = [[0, 4], [1], [2, 3, 0], [4, 2]]
    huge = K(2048) + ["u65"]
    rows = [_time_row("small_speed1", 1.0, small, small_walks),
            _time_row("small_speed1_one_short", 1.0, small, small_walks, short=True),
            _time_row("small_speed0.37_f32", 0.37, small, small_walks, dtype=np.float32),
            _time_row("mid_speed1.6_f32", 1.6, mid, mid_walks, dtype=np.float32),
            _time_row("mid_speed1.6_smoothed", 1.6, mid, mid_walks, smooth=((63, 1), (64, 2), (65, 5), "u2")),
            _time_row("big_speed0.37", 0.37, big, big_walks),
            _time_row("big_speed0.37_smoothed_f32", 0.37, big, big_walks, dtype=np.float32, smooth=((129, 2), (6, 2))),
            _time_row("huge_speed1", 1.0, huge, [[0], [1, 3], [2]])]
    for name, (F, Lt, _, _, _, speed) in tc.CONSTANT.items():
        rows.append(_time_row("constant_" + name, speed, [name, "u64"], [[0], [1, 0], [0, 0, 1]], dtype=np.float32 if name == "count1" else np.float64))
    # rows of 14, 15 and 16 samples of a flagged node: the speed that gives the first step that many (tests/test_gpu_time_smoothing.py's rule)
    for T in (14, 15, 16):
        rows.append(_time_row("smoothed_%d_samples" % T, None, [(65, 2), (64, 1), "u64"], [[0, 2], [1], [2, 0, 1]], smooth=((65, 2),), sized=T))
    refused = [tc.time_model(3, 1, 4, 0.05, 33, name="tw_refused_3"), tc.time_model(2049, 1, 20, 0.05, 2079, name="tw_refused_2049")]
    for data in refused:
        F = data["n_canonical_frames"]
        rows.append(_time_row("F%d_occurs" % F, 1.0, [(5, 1), "u64", ("json", data)], [[0, 1], [2]], expect=UNSUPPORTED))
        rows.append(_time_row("F%d_does_not_occur" % F, 1.0, [(5, 1), "u64", ("json", data)], [[0, 1], [1]]))
    rows.append(dict(_time_row("ld_one_short", 1.0, [(5, 5), "u64"], [[0, 1], [1]], expect=INVALID), ld=tc.N_SPATIAL + 5 - 1))
    return rows


def time_model_of(node):
    """(JSON, gamma rows or None) of a time row's node: a key of timewarp_cases.MODELS / CONSTANT, a name of UNTIMED, or ("json", dict)."""
    if isinstance(node, tuple) and node[0] == "json":
        return node[1], np.zeros((tc.ROWS, len(node[1]["eigen_vectors_time"][0])))
    if node in UNTIMED:
        F = UNTIMED[node]
        return synthetic.make_primitive(seed=12000 + F, n_components=tc.N_SPATIAL, n_frames=F, n_basis=max(4, min(tc.N_BASIS, F + 2)), n_dim=tc.D, n_gmm=1,
                                        name=node), None
    return tc.model_of(node)


MIXED_TIME_ROWS = _time_rows()
TIME_IDS = [r["name"] for r in MIXED_TIME_ROWS]
TIME_BY_NAME = {r["name"]: r for r in MIXED_TIME_ROWS}


def time_case(row):
    """(JSONs, (F, L, Lt) per node, P (n_walks, s_max, ld) of the row's dtype, speed): step (w, i) of a node with a time model holds
    gamma row (w + i) % 3 of timewarp_cases' model in columns L .. L + Lt; every other entry is drawn."""
    jsons, gammas = zip(*[time_model_of(nd) for nd in row["nodes"]])
    shapes = [(int(d["n_canonical_frames"]), tc.N_SPATIAL, len(d["eigen_vectors_time"][0]) if "eigen_vectors_time" in d else 0) for d in jsons]
    node_of, _ = rc.tables(row["walks"])
    P = 0.7 * np.random.default_rng(13000 + TIME_IDS.index(row["name"])).standard_normal(node_of.shape + (row["ld"],))
    for w, seq in enumerate(row["walks"]):
        for i, k in enumerate(seq):
            F, L, Lt = shapes[k]
            if Lt and row["ld"] >= L + Lt:
                P[w, i, L:L + Lt] = gammas[k][(w + i) % tc.ROWS]
    P = P.astype(row["dtype"])
    speed = row["speed"]
    if row["sized"] is not None:                         # num = int(round(t(F - 2)) * (1 / speed)) = T - 2 for the first step of the first walk
        k = row["walks"][0][0]
        c = tc.canonical_time_function(jsons[k], P[0, 0, shapes[k][1]:shapes[k][1] + shapes[k][2]].astype(np.float64))
        speed = float(np.round(c[-2])) / (row["sized"] - 2 + 0.5)
    return list(jsons), shapes, P, speed


@functools.lru_cache(maxsize=None)
def time_reference(name):
    """What both halves hold a time row's steps to, computed once: {(w, i): dict}.  A step of a node with a time model: the host's
    canonical time function of the values the row's dtype holds, FITPACK's row (timewarp_cases.reference_time_function), the 50-digit
    twin's, the count margins, and the tolerance -- timewarp_cases.time_tolerance of the model's (F, Lt, speed) case, or, at a speed
    the case table does not have, its rule on this step's own e_fit.  A step of a node without one: numpy.linspace's row."""
    row = TIME_BY_NAME[name]
    jsons, shapes, P, speed = time_case(row)
    out = {}
    for w, seq in enumerate(row["walks"]):
        for i, k in enumerate(seq):
            F, L, Lt = shapes[k]
            if Lt == 0:
                out[(w, i)] = dict(timed=False, row=np.linspace(0, F, int(F * (1.0 / speed))))
                continue
            c = tc.canonical_time_function(jsons[k], P[w, i, L:L + Lt].astype(np.float64))
            ref, twin = tc.reference_time_function(c, speed), tc.twin_time_function(c, speed)
            cid = time_case_id(row["nodes"][k], speed)
            e_fit = float(np.max(np.abs(ref - twin)))
            tol = tc.time_tolerance(cid) if cid else min(max(16.0 * e_fit, 4.0 * np.spacing(float(F))), 1.0e-11 * F)
            out[(w, i)] = dict(timed=True, canonical=c, row=ref, twin=twin, tol=tol, margins=tc.count_margins(c, speed), case=cid)
    return out


def time_plan(row, t_cap, speed):
    _, shapes, _, _ = time_case(row)
    smooth = None
    if row["smooth"]:
        smooth = [nd in row["smooth"] for nd in row["nodes"]]
    return walks_time_plan(shapes, row["walks"], row["ld"], speed, t_cap, smooth)


def time_case_id(node, speed):
    """The id of timewarp_cases.CASES a timed node's rows are held to at this speed, None where the table has none."""
    cid = node if node in tc.CONSTANT else ("F%d-Lt%d-speed%g" % (node[0], node[1], speed) if isinstance(node, tuple) and node[0] != "json" else None)
    return cid if cid in tc.CASE_IDS and tc.CASES[tc.CASE_IDS.index(cid)][2][5] == speed else None


# ---- the sampler's table ------------------------------------------------------------------------------------------------------------
SAMPLE_F, SAMPLE_NB, SAMPLE_D = 4, 4, 3
LG_LARGEST = largest_sample_width()
# name: ((K, Lg) per node, walks, ld, seed)
_cycle = lambda n, seqs: [list(seqs[w % len(seqs)]) for w in range(n)]
MIXED_SAMPLE_ROWS = {
    "narrow_63_rows": ([(1, 1), (2, 3), (7, 4), (2, 5)], _cycle(21, ([0, 2, 1], [2], [3, 2], [2, 2, 2], [1, 0])), 5, 501),
    "narrow_64_rows_wide_ld": ([(1, 1), (2, 3), (7, 4), (2, 5)], _cycle(32, ([2, 3], [0], [1, 2], [2])), 8, 502),
    "Lg127_65_rows": ([(1, 127), (2, 5)], _cycle(65, ([0], [1], [0])), 127, 503),
    "Lg128_129_rows": ([(2, 128), (7, 4)], _cycle(129, ([0], [1])), 130, 504),
    "largest": ([(1, LG_LARGEST), (2, 3)], [[0, 1], [1], [0]], LG_LARGEST, 505),
    "one_past_the_largest": ([(1, LG_LARGEST + 1), (2, 3)], [[0, 1], [1], [0]], LG_LARGEST + 1, 506),
}
SAMPLE_IDS = sorted(MIXED_SAMPLE_ROWS)
SAMPLE_REFUSED = {"one_past_the_largest": UNSUPPORTED}


@functools.lru_cache(maxsize=None)
def sample_model(K, Lg):
    return synthetic.make_primitive(seed=14000 + 10 * Lg + K, n_components=Lg, n_frames=SAMPLE_F, n_basis=SAMPLE_NB, n_dim=SAMPLE_D, n_gmm=K, name="mix_%d_%d" % (Lg, K))


def sample_plan(name):
    mixtures, walks, ld, _ = MIXED_SAMPLE_ROWS[name]
    return walks_sample_plan(mixtures, walks, ld)


def sample_routes(name):
    mixtures, walks, ld, _ = MIXED_SAMPLE_ROWS[name]
    used = {mixtures[k] for seq in walks for k in seq}
    out = {"sample:K_%d" % K for K, _ in used} | {"sample:Lg_%d" % Lg for _, Lg in used} | {"sample:rows_%d" % (len(walks) * s_max_of(walks))}
    out.add("sample:ld_wider" if ld > max(Lg for _, Lg in mixtures) else "sample:ld_equal")
    if name in SAMPLE_REFUSED:
        return {"refused:sample_lds"}
    plan = sample_plan(name)
    out.add("sample:opt_in" if plan["opt_in"] else "sample:plain_lds")
    if plan["lds"] == MG_WALKS_SAMPLE_LDS_MAX:
        out.add("sample:lds_largest")
    return out | {"sample:float64", "sample:float32", "sample:comp_given", "sample:comp_null"}


# ---- the routes ---------------------------------------------------------------------------------------------------------------------
def time_routes(row):
    out = {"time:speed_%g" % row["speed"] if row["speed"] is not None else "time:smoothed_%d_samples" % row["sized"], "time:lat_%s" % np.dtype(row["dtype"]).name}
    if row["expect"] is not None:
        return {"refused:time_F%d" % row["nodes"][2][1]["n_canonical_frames"] if row["expect"] == UNSUPPORTED else "refused:time_ld"}
    used = {row["nodes"][k] for seq in row["walks"] for k in seq}
    for nd in used:
        if isinstance(nd, tuple) and nd[0] != "json":
            out.add("time:model_F%d_Lt%d" % nd)
        elif nd in tc.CONSTANT:
            out.add("time:constant_" + nd)
        elif nd in UNTIMED:
            out.add("time:untimed_count_%d" % int(UNTIMED[nd] * (1.0 / row["speed"]))) if row["speed"] is not None else None
    if row["short"]:
        out.add("time:one_short")
    if row["smooth"]:
        out.add("time:smoothed")
    if any(isinstance(nd, tuple) and nd[0] == "json" for nd in row["nodes"]):
        out.add("time:unsupported_node_does_not_occur")
    return out


FRAME_ROUTES = set().union(*[r["routes"] for r in MIXED_FRAME_ROWS])
TIME_ROUTES = set().union(*[time_routes(r) for r in MIXED_TIME_ROWS])
SAMPLE_ROUTES = set().union(*[sample_routes(n) for n in SAMPLE_IDS])
MIXED_ROUTES = FRAME_ROUTES | TIME_ROUTES | SAMPLE_ROUTES
