"""mg_step_lengths (csrc/mg_step_length.hip) across its shape edges: an independent reference, the table of shapes, and a ledger of
the boundaries the table straddles.

Shared by tests/test_step_length_shapes_host.py (no device: the layout restated against csrc/mg_step_length_layout.h, the table
against the ledger, the reference against the golden frames, graph_walk._HostModel and a closed form) and
tests/test_gpu_step_length_shapes.py (the same rows on the device).

reference_step_lengths calls nothing of the library: it scales the root rows by translation_maxima, forms the control points, takes
the cubic B-spline basis from the model's own knots by the Cox-de Boor recurrence at the canonical frames, and reduces in extended
precision (np.longdouble where it carries at least 64 mantissa bits, mpmath otherwise); float64 comes in at the very end.

The canonical frames are the reference project's np.linspace(0, F, F) (motion_primitive.py:233), not 0 .. F - 1: the frames of
tests/golden/ are taken there, and the CPU companion holds the reference to them.  The last of them, t = F, lies one frame past the
last knot, where the spline is the end span's polynomial continued (FITPACK's ext = 0).
"""
import numpy as np

from morphablegraphs_amd import _capi, synthetic

MG_ERR_UNSUPPORTED = _capi.MG_ERR_UNSUPPORTED
TILE = 16                              # MG_SLEN_TILE  (pinned to the header and to _capi by the CPU companion)
LDS_MAX = 150 * 1024                   # MG_SLEN_LDS_MAX
KB64 = 64 * 1024
BLOCK = 256                            # threads of a workgroup: the stride of every staging loop
POSITION_BOUND = 4e-12                 # per position, times the scale: what the float64 frames path is held to (test_gpu_step_lengths.py)


def layout_bytes(L, NB, F):
    """mg_slen_layout_of(L, NB, F).total_bytes, restated: E'[L][3 NB], the means, the tap weights, a tile of latents, of control
    points and of segments (rows of F | 1 doubles), then the int32 tail (i0[F], bad[TILE])."""
    return 8 * (3 * L * NB + 3 * NB + 4 * F + TILE * L + TILE * 3 * NB + TILE * (F | 1)) + 4 * (F + TILE)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def _backend(backend):
    if backend is None:
        backend = "longdouble" if np.finfo(np.longdouble).nmant >= 63 else "mpmath"
    if backend == "mpmath":
        import mpmath
        mpmath.mp.prec = 113
        return backend, (lambda a: np.vectorize(mpmath.mpf, otypes=[object])(np.asarray(a, dtype=np.float64))), (lambda a: np.vectorize(mpmath.sqrt, otypes=[object])(a))
    return backend, (lambda a: np.asarray(a, dtype=np.float64).astype(np.longdouble)), np.sqrt


def cox_de_boor(knots, x, zero, one):
    """The NB cubic B-spline basis functions of the knot vector at x, by the recurrence from degree 0 up: N_i,0 = 1 on
    [t_i, t_i+1) -- the last non-empty interval closed at its right end --, N_i,k = (x - t_i) / (t_i+k - t_i) N_i,k-1 +
    (t_i+k+1 - x) / (t_i+k+1 - t_i+1) N_i+1,k-1, a term with an empty support dropped.  An x outside the knots takes the degree-0
    function of the end span, which continues that span's polynomial.  knots and x in the caller's number type."""
    m = len(knots) - 1
    spans = [i for i in range(m) if knots[i] < knots[i + 1]]
    inside = [i for i in spans if knots[i] <= x < knots[i + 1]]
    at = inside[0] if inside else (spans[-1] if x >= knots[spans[-1] + 1] else spans[0])
    N = [one if i == at else zero for i in range(m)]
    for k in range(1, 4):
        nxt = []
        for i in range(m - k):
            v = zero
            if knots[i + k] != knots[i]:
                v = v + (x - knots[i]) / (knots[i + k] - knots[i]) * N[i]
            if knots[i + k + 1] != knots[i + 1]:
                v = v + (knots[i + k + 1] - x) / (knots[i + k + 1] - knots[i + 1]) * N[i + 1]
            nxt.append(v)
        N = nxt
    return N                            # len(knots) - 4 = NB values


def canonical_times(F):
    """the float64 times of the canonical frames: np.linspace(0, F, F) as the reference project takes it"""
    return np.linspace(0, F, int(F))


def reference_root_path(model, S, backend=None):
    """The root positions (n, F, 3) of every row of S at the canonical frames, in the backend's number type."""
    backend, up, _ = _backend(backend)
    NB, D, F = int(model["n_basis_spatial"]), int(model["n_dim_spatial"]), int(model["n_canonical_frames"])
    S = np.atleast_2d(np.asarray(S, dtype=np.float64))
    tm = up(model.get("translation_maxima", (1.0, 1.0, 1.0)))
    mean = up(np.asarray(model["mean_spatial_vector"], dtype=np.float64).reshape(NB, D)[:, :3]) * tm                    # 1. scaled root rows
    eig = up(np.asarray(model["eigen_vectors_spatial"], dtype=np.float64).reshape(S.shape[1], NB, D)[:, :, :3]) * tm
    cp = mean[None] + np.tensordot(up(S), eig, axes=(1, 0))                                                              # 2. (n, NB, 3)
    knots = list(up(np.asarray(model["b_spline_knots_spatial"], dtype=np.float64)))
    assert len(knots) == NB + 4
    zero, one = up(0.0)[()], up(1.0)[()]
    B = np.array([cox_de_boor(knots, up(t)[()], zero, one) for t in canonical_times(F)])                                 # 3. (F, NB)
    return np.tensordot(B, cp, axes=(1, 1)).transpose(1, 0, 2)                                                           # 4. (n, F, 3)


def lengths_of_path(pos, backend=None):
    """(arc length on the ground plane, first-to-last distance) of positions (n, F, 3), rounded to float64 at the end only."""
    _, _, sqrt = _backend(backend)
    d = pos[:, 1:] - pos[:, :-1]
    seg = sqrt(d[:, :, 0] * d[:, :, 0] + d[:, :, 2] * d[:, :, 2])                                                        # 5.
    arc = pos[:, 0, 0] * 0
    for f in range(seg.shape[1]):                                                                                        # 6. in frame order
        arc = arc + seg[:, f]
    e = pos[:, -1] - pos[:, 0]
    dist = sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])                                              # 7.
    return np.array([float(v) for v in arc]), np.array([float(v) for v in dist])                                         # 8.


def reference_step_lengths(model, S, backend=None, with_scale=False):
    """(arc_length (n,), distance (n,)) float64 of the model dict's root path for latents S (n, L); with_scale: and
    max(1, the largest |root coordinate|), the scale the bounds are stated in."""
    pos = reference_root_path(model, S, backend)
    arc, dist = lengths_of_path(pos, backend)
    if with_scale:
        return arc, dist, max(1.0, float(np.max(np.abs(pos))))
    return arc, dist


def arc_bound(F, scale):
    """the bound the project holds the kernel's arc length to against reference frames (tests/test_gpu_step_lengths.py)"""
    return (F - 1) * 2 * np.sqrt(2) * POSITION_BOUND * scale


def dist_bound(scale):
    return 2 * np.sqrt(3) * POSITION_BOUND * scale


def device_bound(F, scale):
    """tests/test_gpu_step_lengths.py's _device_bound: positions that differ in the last bit at both ends of each segment, and a
    sqrt that is not correctly rounded"""
    return max(F - 1, 1) * 8 * 2.0 ** -53 * scale


# ---- the rows -----------------------------------------------------------------------------------------------------------------------
SCALED = (1.5, 2.0, 0.5)               # translation maxima of the rows that have some
ANALYTIC_DIR = (1.5, -0.875)           # the analytic models' path runs along this (x, z) direction ...
ANALYTIC_Y = 91.25                     # ... at this height ...
ANALYTIC_SPEED = 0.75                  # ... and moves this far along it per frame


def _row(name, L, NB, F, D, n, why, tm=(1.0, 1.0, 1.0), kind="plain", expect=None, model_seed=None):
    return dict(name=name, L=L, NB=NB, F=F, D=D, n=n, why=why, tm=tm, kind=kind, expect=expect, model_seed=model_seed)


def _rows():
    rows = [
        _row("F2_NB4", 3, 4, 2, 7, 17, "the fewest frames (t = 0 and t = 2), one segment, and the fewest basis functions: every i0 is 0"),
        _row("F3", 3, 4, 3, 7, 17, "seg[1 .. F-1] of an odd F: FS = F"),
        _row("F12", 5, 7, 12, 7, 17, "even F: FS = F + 1", tm=SCALED),
        _row("F13", 5, 7, 13, 7, 17, "odd F beside F12"),
        _row("F255", 3, 6, 255, 7, 17, "one pass of the frame loops, one frame short of the block"),
        _row("F256", 3, 6, 256, 7, 17, "one pass of the frame loops, exactly the block"),
        _row("F257", 3, 6, 257, 7, 17, "the second pass of the si0 loop: frame 256 is staged by thread 0 again", tm=SCALED),
        _row("NB4_F9", 4, 4, 9, 7, 17, "the fewest basis functions under several frames: one polynomial piece"),
        _row("NB_gt_F", 5, 12, 7, 7, 17, "more basis functions than frames: knots closer than a frame, i0 skips values"),
        _row("L1", 1, 6, 10, 7, 17, "one latent: L * NR = 18, the control points are one fma each"),
        _row("L64", 64, 5, 8, 7, 17, "the widest packed latent width"),
        _row("L65", 65, 5, 8, 7, 17, "past 64 latents"),
        _row("D3", 3, 6, 10, 3, 17, "the fewest channels: the root rows are the whole of E'", tm=SCALED),
        _row("D79", 6, 40, 45, 79, 17, "R = NB * D = 3160: the root rows lie 79 doubles apart"),
        _row("LNR255", 5, 17, 20, 7, 5, "L * NR = ncand * NR = 255: one pass of the E' and control-point loops"),
        _row("LNR258", 2, 43, 50, 7, 2, "L * NR = ncand * NR = 258: a second pass of two threads"),
    ]
    for n in (1, 15, 16, 17, 32, 33):    # one model: the tile's edges
        rows.append(_row("batch_n%d" % n, 5, 7, 12, 7, n, "n = %d of one model against MG_SLEN_TILE = 16" % n, model_seed=11900))
    rows += [
        _row("lds_at_64k", 33, 40, 80, 3, 17, "65 536 bytes exactly: the last size that needs no opt-in"),
        _row("lds_over_64k", 33, 40, 81, 3, 17, "65 572 bytes: the opt-in route through mg_items_launch"),
        _row("lds_at_max", 56, 64, 208, 3, 17, "153 600 bytes exactly: MG_SLEN_LDS_MAX"),
        _row("lds_over_max", 56, 64, 209, 3, 17, "153 636 bytes: refused", expect=MG_ERR_UNSUPPORTED),
        _row("analytic_F13", 5, 7, 13, 7, 17, "zero root eigenvectors, a straight monotone mean path: arc length = distance", tm=SCALED, kind="analytic"),
        _row("analytic_F257", 3, 7, 257, 7, 17, "the same beyond 256 frames", kind="analytic"),
    ]
    for k, r in enumerate(rows):
        r["seed"] = 11000 + 20 * k        # the latents' seed; the model's too unless the row names one
        if r["model_seed"] is None:
            r["model_seed"] = r["seed"] + 1
    return rows


ROWS = _rows()
IDS = [r["name"] for r in ROWS]
BY_NAME = {r["name"]: r for r in ROWS}
LAUNCHED = [r["name"] for r in ROWS if r["expect"] is None]

# one table of five items over three models: a 16-candidate item directly before a 1-candidate one (the wg0 bisection at an exact
# tile boundary), an empty item, a 17 and a 15; (row whose model the item uses, candidates)
MIXED_TABLE = (("F12", 16), ("F257", 1), ("D3", 0), ("F12", 17), ("F257", 15))
# the item over 64 KiB in one table with a tiny one, in both orders: the launch takes the larger size, whichever comes first
LDS_TABLES = {"large_first": (("lds_over_64k", 17), ("F2_NB4", 3)), "small_first": (("F2_NB4", 3), ("lds_over_64k", 17))}


def model_of(row):
    r = BY_NAME[row] if isinstance(row, str) else row
    data = synthetic.make_primitive(seed=r["model_seed"], n_components=r["L"], n_frames=r["F"], n_basis=r["NB"], n_dim=r["D"], n_gmm=1,
                                    translation_maxima=r["tm"], name=r["name"])
    if r["kind"] == "analytic":
        NB, D = r["NB"], r["D"]
        eig = np.array(data["eigen_vectors_spatial"]).reshape(-1, NB, D)
        mean = np.array(data["mean_spatial_vector"]).reshape(NB, D)
        eig[:, :, :3] = 0.0
        u = analytic_abscissae(r)
        mean[:, 0], mean[:, 1], mean[:, 2] = 12.5 + ANALYTIC_DIR[0] * u, ANALYTIC_Y, -3.25 + ANALYTIC_DIR[1] * u
        data["eigen_vectors_spatial"] = eig.reshape(len(eig), -1).tolist()
        data["mean_spatial_vector"] = mean.reshape(-1).tolist()
    return data


def analytic_abscissae(row):
    """u_i = ANALYTIC_SPEED (t_i+1 + t_i+2 + t_i+3) / 3 of the row's knots: the speed times the Greville abscissae, so that by the
    B-spline's linear precision sum_i B_i(t) u_i = ANALYTIC_SPEED t, on the knots and, as an identity of polynomials, past them.
    The rows' knots are whole numbers, so u and its products with ANALYTIC_DIR are exact in float64: the control points are
    collinear exactly and rise strictly."""
    r = BY_NAME[row] if isinstance(row, str) else row
    t = synthetic.cubic_b_spline_knots(r["NB"], r["F"])
    assert np.array_equal(t, np.round(t)) and ANALYTIC_SPEED == 0.75
    return (t[1:-3] + t[2:-2] + t[3:-1]) / 4.0


def analytic_length(row):
    """What both the arc length and the distance are: the path runs straight from t = 0 to t = F (the canonical grid's last
    sample) at ANALYTIC_SPEED along ANALYTIC_DIR, stretched by the translation maxima."""
    r = BY_NAME[row] if isinstance(row, str) else row
    du = np.longdouble(ANALYTIC_SPEED) * r["F"]
    ex, ez = np.longdouble(r["tm"][0] * ANALYTIC_DIR[0]) * du, np.longdouble(r["tm"][2] * ANALYTIC_DIR[1]) * du
    return float(np.sqrt(ex * ex + ez * ez))


def latents_of(row, n=None):
    """The row's latents, float64 values a float32 batch holds exactly (so one set serves both dtypes)."""
    r = BY_NAME[row] if isinstance(row, str) else row
    seed = 11899 if r["name"].startswith("batch_n") else r["seed"]     # the batch rows are prefixes of one matrix
    S = 0.8 * np.random.default_rng(seed).standard_normal((2 * TILE + 1, r["L"]))
    return np.ascontiguousarray(S[:r["n"] if n is None else n].astype(np.float32).astype(np.float64))


def metric(row, what):
    r = BY_NAME[row] if isinstance(row, str) else row
    ncand = min(r["n"], TILE)
    return {"F": r["F"], "F parity": r["F"] & 1, "NB": r["NB"], "L": r["L"], "D": r["D"], "n": r["n"], "bytes": layout_bytes(r["L"], r["NB"], r["F"]),
            "L * NR": r["L"] * 3 * r["NB"], "ncand * NR": ncand * 3 * r["NB"], "4 F": 4 * r["F"], "NB - F": r["NB"] - r["F"],
            "ncand * (F - 1)": ncand * (r["F"] - 1)}[what]


# ---- the ledger: every boundary the sweep exists for, the quantity it is a boundary of, the last value on its near side, and the rows
# (or table items) that lie at or below it and above it.  `at`: a row sits on the edge value itself.
def _b(what, edge, rows, at=True):
    return dict(metric=what, edge=edge, rows=tuple(rows), at=at)


BOUNDARIES = {
    "F: the second pass of the si0 staging loop (256 threads)": _b("F", BLOCK, ("F255", "F256", "F257", "analytic_F257")),
    "F: the passes of the tap-weight staging loop (4 F against 256)": _b("4 F", BLOCK, ("F13", "L64", "D79", "F255"), at=False),
    "F: the fewest frames": _b("F", 2, ("F2_NB4", "F3")),
    "F: both parities of the segment rows' stride F | 1": _b("F parity", 0, ("F12", "F13", "F256", "F257", "lds_at_64k", "lds_over_64k")),
    "NB: the fewest basis functions": _b("NB", 4, ("F2_NB4", "NB4_F9", "F12")),
    "NB: more basis functions than frames": _b("NB - F", 0, ("F12", "NB_gt_F", "F2_NB4"), at=False),
    "L: one latent": _b("L", 1, ("L1", "LNR258")),
    "L: past 64": _b("L", 64, ("L64", "L65")),
    "D: the fewest channels": _b("D", 3, ("D3", "F12", "D79")),
    "L * NR: the passes of the E' staging loop": _b("L * NR", BLOCK, ("L1", "LNR255", "LNR258", "L64"), at=False),
    "ncand * NR: the passes of the control-point loop": _b("ncand * NR", BLOCK, ("batch_n1", "LNR255", "LNR258", "batch_n17"), at=False),
    "ncand * (F - 1): the passes of the segment loop": _b("ncand * (F - 1)", BLOCK, ("F2_NB4", "batch_n17", "F257"), at=False),
    "n: the tile": _b("n", TILE, ("batch_n1", "batch_n15", "batch_n16", "batch_n17")),
    "n: two tiles": _b("n", 2 * TILE, ("batch_n32", "batch_n33")),
    "LDS: the 64 KiB opt-in": _b("bytes", KB64, ("lds_at_64k", "lds_over_64k")),
    "LDS: the refusal at MG_SLEN_LDS_MAX": _b("bytes", LDS_MAX, ("lds_at_max", "lds_over_max")),
    "LDS: items of one launch on both sides of 64 KiB": _b("bytes", KB64, [name for name, _ in LDS_TABLES["large_first"]], at=False),
}

# what the device sweep must have run and matched before its last test passes
LEDGER_WANT = set(IDS) | {"table:mixed"} | {"table:%s:%s%s" % (order, dt, fresh) for order in LDS_TABLES for dt in ("float32", "float64") for fresh in ("", ":fresh")}
