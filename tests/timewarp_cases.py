"""The cases of the time-warp tests and the plain statements they are held to (no test in here: tests/test_timewarp_host.py checks
this module on the CPU, tests/test_gpu_timewarp_shapes.py runs the kernels of csrc/mg_timewarp.hip against it).

A case is (F, Lt, n_basis_time, amplitude, gamma rows, speed): a time model of F canonical frames and Lt time components whose
log-increments are about N(0, amplitude^2) (or constant, see CONSTANT), `gamma rows` standard-normal time latents, one speed.
The spatial part is tiny (D = 11, 6 control points, 3 components).  Every model's seed was chosen on the CPU so that every row of
every one of its cases is safe for an exact comparison of the sample count (count_margins)."""
import functools

import numpy as np
from scipy.interpolate import splev, splrep

from morphablegraphs_amd import synthetic

D, N_BASIS, N_SPATIAL = 11, 6, 3
FRAMES = (4, 5, 6, 63, 64, 65, 129, 2048)       # the m == 4 solve, neighbouring end rows, the 64-lane stride, MG_TW_MAX_F
TIME_COMPONENTS = (1, 2, 5)
SPEEDS = (1.0, 1.6, 0.37)
ROWS = 3
MARGIN = 1.0e-6

# (F, Lt) -> (n_basis_time, amplitude, seed)
MODELS = {}
_SEEDS = {(4, 1): 400, (4, 2): 436, (4, 5): 402, (5, 1): 500, (5, 2): 501, (5, 5): 502, (6, 1): 600, (6, 2): 601, (6, 5): 602,
          (63, 1): 6300, (63, 2): 6301, (63, 5): 6302, (64, 1): 6400, (64, 2): 6408, (64, 5): 6402, (65, 1): 6500, (65, 2): 6501, (65, 5): 6502,
          (129, 1): 12900, (129, 2): 12901, (129, 5): 12909, (2048, 1): 204800, (2048, 2): 204801, (2048, 5): 204809}
for _F in FRAMES:
    for _Lt in TIME_COMPONENTS:
        MODELS[(_F, _Lt)] = (4 if _F <= 5 else (5 if _F <= 6 else (8 if _F < 2048 else 20)), 0.5 if _Lt == 2 else 0.05, _SEEDS[(_F, _Lt)])

# models with a CONSTANT log-increment c (a constant mean_time_vector: the B-spline basis sums to one) and harmonics of 1e-3:
# name -> (F, Lt, n_basis_time, c, seed, speed)
CONSTANT = {
    "count0": (4, 1, 4, 0.0, 410, 3.0),                  # round(t(2)) = 2, 2 * (1 / 3) < 1: no inner sample
    "count1": (4, 1, 4, 0.0, 410, 1.6),                  # 2 * 0.625 = 1.25: one inner sample, step 0
    "first_sample_below_x0": (6, 2, 5, float(np.log(2.6)), 610, 1.0),   # x[0] = 1.6 > t = 1: the first piece outside its interval
    "long_row": (64, 1, 8, 1.5, 6410, 1.0),              # about 281 samples: more than 4 F + 8 = 264
}


def time_model(F, Lt, n_basis_time, amplitude, seed, constant=None, name=None):
    """The reference's legacy JSON of a primitive with a time model, built directly."""
    data = synthetic.make_primitive(seed=seed, n_components=N_SPATIAL, n_frames=F, n_basis=N_BASIS, n_dim=D, n_gmm=2,
                                    name=name or "tw_%d_%d" % (F, Lt), n_time_components=Lt, n_basis_time=n_basis_time)
    rng = np.random.default_rng(seed + 1)
    data["eigen_vectors_time"] = (amplitude / np.sqrt(Lt) * rng.standard_normal((n_basis_time, Lt))).tolist()
    if constant is None:
        data["mean_time_vector"] = (0.5 * amplitude * rng.standard_normal(n_basis_time)).tolist()
    else:
        data["mean_time_vector"] = [float(constant)] * n_basis_time
    return data


@functools.lru_cache(maxsize=None)
def model_of(key):
    """(JSON, gamma (ROWS, Lt)) of MODELS[(F, Lt)] or CONSTANT[name]."""
    if key in CONSTANT:
        F, Lt, nbt, c, seed, _ = CONSTANT[key]
        data = time_model(F, Lt, nbt, 1.0e-3, seed, constant=c, name="tw_" + key)
    else:
        F, Lt = key
        nbt, amplitude, seed = MODELS[key]
        data = time_model(F, Lt, nbt, amplitude, seed)
    gamma = np.random.default_rng(seed + 2).standard_normal((ROWS, Lt))
    return data, gamma


def case_table():
    """[(id, model key, (F, Lt, n_basis_time, amplitude, gamma rows, speed))]"""
    out = []
    for (F, Lt), (nbt, amplitude, _) in MODELS.items():
        for speed in SPEEDS:
            out.append(("F%d-Lt%d-speed%g" % (F, Lt, speed), (F, Lt), (F, Lt, nbt, amplitude, ROWS, speed)))
    for name, (F, Lt, nbt, c, _, speed) in CONSTANT.items():
        out.append((name, name, (F, Lt, nbt, 1.0e-3, ROWS, speed)))
    return out


CASES = case_table()
CASE_IDS = [c[0] for c in CASES]


# ---- the plain statements ------------------------------------------------------------------------------------------------
def canonical_time_function(data, gamma):
    """t(t') at the canonical frames, the reference's statements (motion_primitive.py:289-302): the running sum of
    exp(mean spline + harmonics . gamma) in canonical-frame order, minus 1."""
    F = int(data["n_canonical_frames"])
    knots, frames = np.asarray(data["b_spline_knots_time"], dtype=np.float64), np.arange(F)
    mean_t = splev(frames, (knots, np.asarray(data["mean_time_vector"], dtype=np.float64), 3))
    eig = np.asarray(data["eigen_vectors_time"], dtype=np.float64)
    phi = np.array([splev(frames, (knots, eig[:, l].copy(), 3)) for l in range(eig.shape[1])]).T
    out = [0]
    for i in range(F):
        out.append(out[-1] + np.exp(mean_t[i] + np.dot(phi[i], gamma)))
    return np.array(out[1:]) - 1.0


def sample_count(canonical, speed):
    return max(int(np.round(canonical[-2]) * (1.0 / speed)), 0)


def sample_points(canonical, speed):
    return np.linspace(1, canonical[-2], sample_count(canonical, speed))


def reference_time_function(canonical, speed):
    """The reference's _invert_canonical_to_sample_time_function (motion_primitive.py:304-319): FITPACK's interpolating cubic
    through (t(t'), t') at linspace(1, t(F - 2), num) between the pinned ends; the float `num` truncated with int() (what
    NumPy < 1.18 made of it); no inner sample: the two ends."""
    canonical = np.asarray(canonical, dtype=np.float64)
    F = len(canonical)
    if sample_count(canonical, speed) == 0:
        return np.array([0.0, F - 1.0])
    inner = splev(sample_points(canonical, speed), splrep(canonical, np.arange(F), w=None, k=3))
    return np.concatenate(([0.0], inner, [F - 1.0]))


def count_margins(canonical, speed):
    """(distance of t(F - 2) from a half-integer, distance of round(t(F - 2)) * (1 / speed) from an integer): with both >= MARGIN
    a last-bit difference of the device's exp() cannot move the sample count.  At a speed whose inverse is an integer the product
    IS an integer in every arithmetic (an exact integer times an exact integer): the second distance is reported as inf there."""
    last = float(canonical[-2])
    half = abs(abs(last - np.floor(last)) - 0.5)
    inv = 1.0 / speed
    prod = np.round(last) * inv
    whole = np.inf if inv == np.floor(inv) else abs(prod - np.round(prod))
    return half, whole


# ---- the high-precision twin ---------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def _not_a_knot_system(x):
    """Rows {column: value} and right-hand side of the not-a-knot cubic's second derivatives through (x_i, i), 50 digits."""
    mp = _mp()
    F = len(x)
    h = [x[i + 1] - x[i] for i in range(F - 1)]
    rows, rhs = [], []
    rows.append({0: h[1], 1: -(h[0] + h[1]), 2: h[0]})                     # the third derivative is continuous at x_1
    rhs.append(mp.mpf(0))
    for i in range(1, F - 1):
        rows.append({i - 1: h[i - 1], i: 2 * (h[i - 1] + h[i]), i + 1: h[i]})
        rhs.append(6 * (1 / h[i] - 1 / h[i - 1]))                           # ordinates 0 .. F - 1: every rise is 1
    rows.append({F - 3: h[F - 2], F - 2: -(h[F - 3] + h[F - 2]), F - 1: h[F - 3]})   # ... and at x_{F-2}
    rhs.append(mp.mpf(0))
    return rows, rhs


def second_derivatives_mp(canonical, dense):
    """The twin's second derivatives: dense=True by mpmath's dense LU solve, dense=False by elimination inside the band (the
    system has two sub- and two super-diagonals), which is what F = 2048 can afford; tests/test_timewarp_host.py holds the two
    to each other and checks the band solution's residual."""
    mp = _mp()
    x = [mp.mpf(float(v)) for v in canonical]
    F = len(x)
    rows, rhs = _not_a_knot_system(x)
    if dense:
        A = mp.matrix(F, F)
        for i, r in enumerate(rows):
            for j, v in r.items():
                A[i, j] = v
        sol = mp.lu_solve(A, mp.matrix(rhs))
        return x, [sol[i] for i in range(F)]
    rows, rhs = [dict(r) for r in rows], list(rhs)
    for p in range(F):                                                       # forward elimination; rows p + 1, p + 2 can hold column p
        piv = rows[p][p]
        for i in range(p + 1, min(p + 3, F)):
            f = rows[i].pop(p, None)
            if f is None:
                continue
            f = f / piv
            for j, v in rows[p].items():
                if j > p:
                    rows[i][j] = rows[i].get(j, 0) - f * v
            rhs[i] = rhs[i] - f * rhs[p]
    M = [None] * F
    for p in range(F - 1, -1, -1):
        M[p] = (rhs[p] - sum(v * M[j] for j, v in rows[p].items() if j > p)) / rows[p][p]
    return x, M


def residual_mp(canonical, M):
    """Largest |row . M - right-hand side| of the not-a-knot system."""
    mp = _mp()
    rows, rhs = _not_a_knot_system([mp.mpf(float(v)) for v in canonical])
    return max(abs(sum(v * M[j] for j, v in r.items()) - b) for r, b in zip(rows, rhs))


def twin_time_function(canonical, speed, dense=None):
    """reference_time_function in 50 digits: the not-a-knot cubic through (t(t'), t') evaluated at the same (float64) sample points."""
    mp = _mp()
    canonical = np.asarray(canonical, dtype=np.float64)
    F = len(canonical)
    if sample_count(canonical, speed) == 0:
        return np.array([0.0, F - 1.0])
    x, M = second_derivatives_mp(canonical, F <= 6 if dense is None else dense)
    out = [0.0]
    for t in sample_points(canonical, speed):
        i = min(max(int(np.searchsorted(canonical, t, side="right")) - 1, 0), F - 2)
        t = mp.mpf(float(t))
        h, a, b = x[i + 1] - x[i], x[i + 1] - t, t - x[i]
        out.append(float(M[i] * a ** 3 / (6 * h) + M[i + 1] * b ** 3 / (6 * h) + (i / h - M[i] * h / 6) * a + ((i + 1) / h - M[i + 1] * h / 6) * b))
    return np.array(out + [F - 1.0])


@functools.lru_cache(maxsize=None)
def case_figures(case_id):
    """(e_fit, smallest half-integer margin, smallest integer margin, sample counts) of a case over its gamma rows: e_fit is
    FITPACK's largest deviation from the twin, in canonical frames."""
    _, key, (F, Lt, nbt, amplitude, rows, speed) = CASES[CASE_IDS.index(case_id)]
    data, gamma = model_of(key)
    e_fit, half, whole, counts = 0.0, np.inf, np.inf, []
    for g in gamma:
        c = canonical_time_function(data, g)
        e_fit = max(e_fit, float(np.max(np.abs(reference_time_function(c, speed) - twin_time_function(c, speed)))))
        m = count_margins(c, speed)
        half, whole = min(half, m[0]), min(whole, m[1])
        counts.append(sample_count(c, speed))
    return e_fit, half, whole, counts


def time_tolerance(case_id):
    """max(16 e_fit, 4 ulp of F), never above the suite's 1e-11 F: 16 x for another valid float64 evaluation order
    (second derivatives against FITPACK's B-spline form) of a result whose own rounding error is e_fit."""
    F = CASES[CASE_IDS.index(case_id)][2][0]
    return min(max(16.0 * case_figures(case_id)[0], 4.0 * np.spacing(float(F))), 1.0e-11 * F)
