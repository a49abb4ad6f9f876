"""Random graph walks: a population in which every walk has its own node sequence.

MotionStateGraph.generate_random_walk (reference motion_model/motion_state_graph.py:52-71) picks a random start state of an
action, MotionStateGroup.generate_random_walk (motion_state_group.py:177-214) follows random standard transitions and closes with
an end transition, and every step's parameters are one draw from its node's mixture (:107-129).  Here

  choose_random_walks      the node sequences, the reference's rule and its calls of `random` in its order;
  sample_walk_latents      every step's parameters of the whole population in ONE launch (mg_walks_sample_latents);
  RandomWalks.frames       every walk's motion in TWO launches (mg_walks_frames, csrc/mg_walks_mixed.hip), where
                           graph_walk.assemble_walks serves walks over one sequence and would take a call per distinct sequence;
                           with use_time_parameters the time-warped motion the reference hands back from a finished walk
                           (back_project(s, True) per step): every step's time row in ONE launch (mg_walks_time_functions, the
                           time latents read where the sampler left them), one download of the lengths, the frames at those
                           times in TWO launches (mg_walks_frames_at);
  assemble_walks_mixed_host  the NumPy statement of the frames: graph_walk.assemble_walk_host walk by walk;
  walk_time_rows_host      the NumPy statement of the time rows.

Out of scope: parameters predicted by transition models (the predictor class is not in the reference tree) and smoothed time
functions (smooth_time_parameters) of a primitive that does not opt in with smooth_on_device (NotImplementedError; with it the
Savitzky-Golay pass runs inside mg_walks_time_functions_smoothed).
"""
import ctypes as C
import random

import numpy as np

from . import _capi
from .graph_walk import HipGraphWalk, HipGraphWalkStep, _primitive_of, _untimed_grid, assemble_walk_host
from .motion_state_graph import NODE_TYPE_END, NODE_TYPE_STANDARD, random_edge


# ---- the node sequences ----------------------------------------------------------------------------------------------
def _start_states(graph, action):
    if action not in graph.node_groups:
        raise KeyError("the graph has no action %r" % (action,))
    group = graph.node_groups[action]
    info = group["info"] if isinstance(group, dict) else group
    states = info.get("start_states", []) if isinstance(info, dict) else info.start_states
    if len(states) == 0:
        raise ValueError("action %r has no start state" % (action,))
    return states


def _transition(node, transition_type, rng):
    return random_edge(node.outgoing_edges, lambda key: node.outgoing_edges[key].transition_type == transition_type, rng)


def choose_random_walks(graph, start_action, number_of_steps, n_walks=1, rng=None):
    """The node keys of n_walks random walks, a list per walk: a random start state of the action; then, if that node has
    standard transitions, number_of_steps random standard transitions; then one end transition if the last node has one.
    rng: a random.Random (default: the global `random`, as in the reference), consumed in the reference's order --
    randrange(0, n, 1) over the start states, then over the matching edges in outgoing_edges order; a node without a matching
    edge draws nothing."""
    rng = random if rng is None else rng
    states = _start_states(graph, start_action)
    walks = []
    for _ in range(int(n_walks)):
        current = (start_action, states[rng.randrange(0, len(states), 1)])
        if current not in graph.nodes:
            raise KeyError("start state %r is not a node of the graph" % (current,))
        keys = [current]
        if graph.nodes[current].n_standard_transitions > 0:
            for _ in range(int(number_of_steps)):
                current = _transition(graph.nodes[current], NODE_TYPE_STANDARD, rng)
                if current is None:      # (the reference fails on the missing key in its next line)
                    raise ValueError("node %r counts standard transitions it does not have" % (keys[-1],))
                keys.append(current)
        end = _transition(graph.nodes[current], NODE_TYPE_END, rng)
        if end is not None:
            keys.append(end)
        walks.append(keys)
    return walks


def has_transition_models(graph, action):
    """MotionStateGroup.has_transition_models: an edge out of a node of the action carries a transition model."""
    return any(getattr(edge, "transition_model", None) is not None
               for key, node in graph.nodes.items() if key[0] == action for edge in node.outgoing_edges.values())


# ---- the tables -----------------------------------------------------------------------------------------------------
def walk_tables(node_keys, known=None):
    """(nodes, node_of, n_steps) of a population: the node keys that occur, in order of first occurrence; node_of int32
    (n_walks, s_max) indices into them, -1 behind a walk's end; n_steps int32 (n_walks).  known: the graph's keys, checked."""
    if len(node_keys) == 0:
        raise ValueError("a population of no walks")
    nodes, index = [], {}
    n_steps = np.array([len(keys) for keys in node_keys], dtype=np.int32)
    if n_steps.min() < 1:
        raise ValueError("walk %d has no step" % int(np.argmin(n_steps)))
    node_of = np.full((len(node_keys), int(n_steps.max())), -1, dtype=np.int32)
    for w, keys in enumerate(node_keys):
        for i, key in enumerate(keys):
            key = tuple(key) if isinstance(key, list) else key
            if known is not None and key not in known:
                raise KeyError("walk %d, step %d: %r is not a node of the graph" % (w, i, key))
            if key not in index:
                index[key] = len(nodes)
                nodes.append(key)
            node_of[w, i] = index[key]
    return nodes, node_of, n_steps


def _handles(prims):
    return (C.c_void_p * len(prims))(*[p.handle.value for p in prims])


def sample_walk_latents_dev(prims, node_of, n_steps, seed, d_x, dtype, ld, d_component=None):
    """mg_walks_sample_latents on device buffers: d_x (n_walks, s_max, ld) of dtype, d_component int32 (n_walks, s_max) or None."""
    node_of, n_steps = np.ascontiguousarray(node_of, dtype=np.int32), np.ascontiguousarray(n_steps, dtype=np.int32)
    code = _capi.MG_F64 if np.dtype(dtype) == np.float64 else _capi.MG_F32
    _capi._check(prims[0].lib.mg_walks_sample_latents(len(prims), _handles(prims), _capi._host_ptr(node_of), _capi._host_ptr(n_steps), node_of.shape[0],
                                                      node_of.shape[1], C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _capi._dev_ptr(d_x), code, int(ld),
                                                      _capi._dev_ptr(d_component) if d_component is not None else None))


def sample_walk_latents(prims, node_of, n_steps, seed, dtype=np.float64, ld=None):
    """The same draw into host arrays (mg_walks_sample_latents_host): (x (n_walks, s_max, ld), component (n_walks, s_max))."""
    node_of, n_steps = np.ascontiguousarray(node_of, dtype=np.int32), np.ascontiguousarray(n_steps, dtype=np.int32)
    ld = max(p.n_gmm_dims for p in prims) if ld is None else int(ld)
    x = np.empty(node_of.shape + (ld,), dtype=dtype)
    comp = np.empty(node_of.shape, dtype=np.int32)
    _capi._check(prims[0].lib.mg_walks_sample_latents_host(len(prims), _handles(prims), _capi._host_ptr(node_of), _capi._host_ptr(n_steps), node_of.shape[0],
                                                           node_of.shape[1], C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _capi._host_ptr(x),
                                                           _capi._dtype_code(x), ld, _capi._host_ptr(comp)))
    return x, comp


def _frames_args(prims, node_of, n_steps, frame_offset, alignment, skeleton):
    node_of, n_steps = np.ascontiguousarray(node_of, dtype=np.int32), np.ascontiguousarray(n_steps, dtype=np.int32)
    fo = None if frame_offset is None else np.ascontiguousarray(frame_offset, dtype=np.int64)
    al = _capi.ConstraintSet._marshal_alignment(alignment, skeleton) if alignment is not None else None
    sk = skeleton.desc() if skeleton is not None else None
    return node_of, n_steps, fo, al, sk


def walks_frames_dev(prims, node_of, n_steps, d_latents, dtype, ld, d_frames, walk_stride, frame_offset=None, alignment=None, skeleton=None,
                     d_transforms=None):
    """mg_walks_frames on device buffers.  node_of (n_walks, s_max), n_steps (n_walks), frame_offset None or (n_walks, s_max): host."""
    node_of, n_steps, fo, al, sk = _frames_args(prims, node_of, n_steps, frame_offset, alignment, skeleton)
    code = _capi.MG_F64 if np.dtype(dtype) == np.float64 else _capi.MG_F32
    _capi._check(prims[0].lib.mg_walks_frames(len(prims), _handles(prims), _capi._host_ptr(node_of), _capi._host_ptr(n_steps), _capi._dev_ptr(d_latents), code,
                                              node_of.shape[0], node_of.shape[1], int(ld), _capi._host_ptr(fo), C.byref(al) if al is not None else None,
                                              C.byref(sk) if sk is not None else None, _capi._dev_ptr(d_frames), int(walk_stride),
                                              _capi._dev_ptr(d_transforms) if d_transforms is not None else None))


def walks_frames_host(prims, node_of, n_steps, latents, frames, frame_offset=None, alignment=None, skeleton=None, transforms=None):
    """mg_walks_frames_host: latents (n_walks, s_max, ld) float32 / float64, frames (n_walks, walk_stride, n_dim) float64 written in
    place (rows no step owns keep their values), transforms None or (n_walks, s_max, 4) float64 written in place."""
    node_of, n_steps, fo, al, sk = _frames_args(prims, node_of, n_steps, frame_offset, alignment, skeleton)
    latents = _capi._latents(latents.reshape(-1, latents.shape[-1])).reshape(latents.shape)
    assert frames.dtype == np.float64 and frames.flags.c_contiguous and (transforms is None or (transforms.dtype == np.float64 and transforms.flags.c_contiguous))
    _capi._check(prims[0].lib.mg_walks_frames_host(len(prims), _handles(prims), _capi._host_ptr(node_of), _capi._host_ptr(n_steps), _capi._host_ptr(latents),
                                                   _capi._dtype_code(latents), node_of.shape[0], node_of.shape[1], latents.shape[-1], _capi._host_ptr(fo),
                                                   C.byref(al) if al is not None else None, C.byref(sk) if sk is not None else None,
                                                   _capi._host_ptr(frames), frames.shape[1], _capi._host_ptr(transforms)))


def walks_time_functions_dev(prims, node_of, n_steps, d_latents, dtype, ld, speed, d_times, d_lengths, t_cap):
    """mg_walks_time_functions on device buffers: d_times (n_walks, s_max, t_cap) float64, d_lengths int32 (n_walks, s_max)."""
    node_of, n_steps = np.ascontiguousarray(node_of, dtype=np.int32), np.ascontiguousarray(n_steps, dtype=np.int32)
    code = _capi.MG_F64 if np.dtype(dtype) == np.float64 else _capi.MG_F32
    _capi._check(prims[0].lib.mg_walks_time_functions(len(prims), _handles(prims), _capi._host_ptr(node_of), _capi._host_ptr(n_steps), _capi._dev_ptr(d_latents),
                                                      code, node_of.shape[0], node_of.shape[1], int(ld), float(speed), _capi._dev_ptr(d_times),
                                                      _capi._dev_ptr(d_lengths), int(t_cap)))


def walks_time_functions_smoothed_dev(prims, node_of, n_steps, smooth_of_node, d_latents, dtype, ld, speed, d_times, d_lengths, t_cap):
    """mg_walks_time_functions_smoothed on device buffers: walks_time_functions_dev with smooth_of_node, one flag per node (host)."""
    node_of, n_steps = np.ascontiguousarray(node_of, dtype=np.int32), np.ascontiguousarray(n_steps, dtype=np.int32)
    smooth = np.ascontiguousarray(np.asarray(smooth_of_node).astype(bool), dtype=np.uint8)
    assert len(smooth) == len(prims)
    code = _capi.MG_F64 if np.dtype(dtype) == np.float64 else _capi.MG_F32
    _capi._check(prims[0].lib.mg_walks_time_functions_smoothed(len(prims), _handles(prims), _capi._host_ptr(node_of), _capi._host_ptr(n_steps), _capi._host_ptr(smooth),
                                                               _capi._dev_ptr(d_latents), code, node_of.shape[0], node_of.shape[1], int(ld), float(speed),
                                                               _capi._dev_ptr(d_times), _capi._dev_ptr(d_lengths), int(t_cap)))


def walks_time_functions_smoothed_host(prims, node_of, n_steps, smooth_of_node, latents, speed, times, lengths):
    """mg_walks_time_functions_smoothed_host: walks_time_functions_host with smooth_of_node, one flag per node."""
    node_of, n_steps = np.ascontiguousarray(node_of, dtype=np.int32), np.ascontiguousarray(n_steps, dtype=np.int32)
    smooth = np.ascontiguousarray(np.asarray(smooth_of_node).astype(bool), dtype=np.uint8)
    assert len(smooth) == len(prims)
    latents = _capi._latents(latents.reshape(-1, latents.shape[-1])).reshape(latents.shape)
    assert times.dtype == np.float64 and times.flags.c_contiguous and lengths.dtype == np.int32 and lengths.flags.c_contiguous
    _capi._check(prims[0].lib.mg_walks_time_functions_smoothed_host(len(prims), _handles(prims), _capi._host_ptr(node_of), _capi._host_ptr(n_steps),
                                                                    _capi._host_ptr(smooth), _capi._host_ptr(latents), _capi._dtype_code(latents), node_of.shape[0],
                                                                    node_of.shape[1], latents.shape[-1], float(speed), _capi._host_ptr(times),
                                                                    _capi._host_ptr(lengths), times.shape[2]))


def walks_time_functions_host(prims, node_of, n_steps, latents, speed, times, lengths):
    """mg_walks_time_functions_host: latents (n_walks, s_max, ld) float32 / float64; times (n_walks, s_max, t_cap) float64 and
    lengths (n_walks, s_max) int32 written in place (rows that are not written keep their values)."""
    node_of, n_steps = np.ascontiguousarray(node_of, dtype=np.int32), np.ascontiguousarray(n_steps, dtype=np.int32)
    latents = _capi._latents(latents.reshape(-1, latents.shape[-1])).reshape(latents.shape)
    assert times.dtype == np.float64 and times.flags.c_contiguous and lengths.dtype == np.int32 and lengths.flags.c_contiguous
    _capi._check(prims[0].lib.mg_walks_time_functions_host(len(prims), _handles(prims), _capi._host_ptr(node_of), _capi._host_ptr(n_steps), _capi._host_ptr(latents),
                                                           _capi._dtype_code(latents), node_of.shape[0], node_of.shape[1], latents.shape[-1], float(speed),
                                                           _capi._host_ptr(times), _capi._host_ptr(lengths), times.shape[2]))


def walks_frames_at_dev(prims, node_of, n_steps, d_latents, dtype, ld, d_times, lengths, t_cap, frame_offset, d_frames, walk_stride, alignment=None,
                        skeleton=None, d_transforms=None):
    """mg_walks_frames_at on device buffers.  d_times (n_walks, s_max, t_cap); lengths int32 and frame_offset int64 (n_walks, s_max): host."""
    node_of, n_steps, fo, al, sk = _frames_args(prims, node_of, n_steps, frame_offset, alignment, skeleton)
    ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
    code = _capi.MG_F64 if np.dtype(dtype) == np.float64 else _capi.MG_F32
    _capi._check(prims[0].lib.mg_walks_frames_at(len(prims), _handles(prims), _capi._host_ptr(node_of), _capi._host_ptr(n_steps), _capi._dev_ptr(d_latents), code,
                                                 node_of.shape[0], node_of.shape[1], int(ld), _capi._dev_ptr(d_times) if d_times is not None else None,
                                                 _capi._host_ptr(ln), int(t_cap), _capi._host_ptr(fo), C.byref(al) if al is not None else None,
                                                 C.byref(sk) if sk is not None else None, _capi._dev_ptr(d_frames), int(walk_stride),
                                                 _capi._dev_ptr(d_transforms) if d_transforms is not None else None))


def walks_frames_at_host(prims, node_of, n_steps, latents, times, lengths, frame_offset, frames, alignment=None, skeleton=None, transforms=None):
    """mg_walks_frames_at_host: times (n_walks, s_max, t_cap) float64; the rest as walks_frames_host."""
    node_of, n_steps, fo, al, sk = _frames_args(prims, node_of, n_steps, frame_offset, alignment, skeleton)
    latents = _capi._latents(latents.reshape(-1, latents.shape[-1])).reshape(latents.shape)
    times, ln = np.ascontiguousarray(times, dtype=np.float64), np.ascontiguousarray(lengths, dtype=np.int32)
    assert frames.dtype == np.float64 and frames.flags.c_contiguous and (transforms is None or (transforms.dtype == np.float64 and transforms.flags.c_contiguous))
    _capi._check(prims[0].lib.mg_walks_frames_at_host(len(prims), _handles(prims), _capi._host_ptr(node_of), _capi._host_ptr(n_steps), _capi._host_ptr(latents),
                                                      _capi._dtype_code(latents), node_of.shape[0], node_of.shape[1], latents.shape[-1], _capi._host_ptr(times),
                                                      _capi._host_ptr(ln), times.shape[2], _capi._host_ptr(fo), C.byref(al) if al is not None else None,
                                                      C.byref(sk) if sk is not None else None, _capi._host_ptr(frames), frames.shape[1],
                                                      _capi._host_ptr(transforms)))


# ---- the frames on the host ---------------------------------------------------------------------------------------------
def _time_model_of(model):
    """feature_point_model._time_model_host's (knots, mean vector, eigen vectors) of a node's model, None without a time model."""
    from .feature_point_model import _time_model_host
    if isinstance(model, dict):
        return _time_model_host(model) if "eigen_vectors_time" in model and len(model["eigen_vectors_time"]) else None
    mp = getattr(model, "motion_primitive", model)
    return _time_model_host(mp) if mp.has_time_parameters and mp.get_n_time_components() > 0 else None


def walk_time_rows_host(models, node_of, n_steps, parameters, speed=1.0, smooth=None):
    """The NumPy statement of mg_walks_time_functions: times[w][i], the time row of step i of walk w.  models: one per node (JSON
    dicts or primitives); parameters (n_walks, s_max, ld).  A node with a time model reads gamma from columns n_components ..
    n_components + n_time_components of the step's row: feature_point_model's canonical_time_function_host and its inverse,
    sample_time_function_host, at `speed` (ValueError where the time function is not finite).  A node without one:
    graph_walk._untimed_grid, linspace(0, F, int(F * (1 / speed))).  smooth: None, or one flag per node -- the rows of a flagged node
    with a time model pass through time_smoothing.smooth_time_row_host, the statement of mg_walks_time_functions_smoothed
    (ValueError for a row of fewer than 15 samples)."""
    from .feature_point_model import canonical_time_function_host, sample_time_function_host
    from .time_smoothing import smooth_time_row_host
    from .graph_walk import _HostModel, _untimed_grid
    hosts = [m if isinstance(m, _HostModel) else _HostModel(m) for m in models]
    time_models = [_time_model_of(m) for m in models]
    parameters = np.asarray(parameters, dtype=np.float64)
    times = []
    for w, ns in enumerate(np.asarray(n_steps)):
        rows = []
        for i, k in enumerate(np.asarray(node_of)[w, :ns]):
            hm, tm = hosts[k], time_models[k]
            if tm is None:
                rows.append(_untimed_grid(hm.n_canonical_frames, speed))
                continue
            gamma = parameters[w, i, hm.n_components:hm.n_components + tm[2].shape[1]]
            row = sample_time_function_host(canonical_time_function_host(tm, hm.n_canonical_frames, gamma), speed)
            if row is None:
                raise ValueError("a time function is not finite")
            rows.append(smooth_time_row_host(row) if smooth is not None and smooth[k] else row)
        times.append(rows)
    return times


def assemble_walks_mixed_host(models, node_of, n_steps, parameters, alignment=None, skeleton=None, times=None, speed=1.0):
    """The NumPy statement of mg_walks_frames: graph_walk.assemble_walk_host for every walk on its own.  models: one per node
    (JSON dicts or primitives); parameters (n_walks, s_max, ld), step (w, i) reads the first n_components columns of its row.
    times: None (canonical grids) or times[w][i], the step's time row (walk_time_rows_host; None for a step: its canonical grid
    at `speed`) -- the statement of mg_walks_frames_at.
    Returns (frames: a list of (T_w, D) arrays, offsets: a list of (n_steps[w] + 1) arrays, transforms (n_walks, s_max, 4), NaN
    for the steps a walk does not have)."""
    from .graph_walk import _HostModel
    models = [m if isinstance(m, _HostModel) else _HostModel(m) for m in models]
    parameters = np.asarray(parameters, dtype=np.float64)
    frames, offsets, transforms = [], [], np.full(parameters.shape[:2] + (4,), np.nan)
    for w, ns in enumerate(np.asarray(n_steps)):
        steps = [models[k] for k in np.asarray(node_of)[w, :ns]]
        S = np.concatenate([parameters[w, i, :m.n_components] for i, m in enumerate(steps)])[None, :]
        fr, offs, tr = assemble_walk_host(steps, S, times=None if times is None else [times[w]], alignment=alignment, skeleton=skeleton, speed=speed)
        frames.append(fr[0])
        offsets.append(offs[0])
        transforms[w, :ns] = tr[0]
    return frames, offsets, transforms


# ---- the population --------------------------------------------------------------------------------------------------------
class RandomWalks(object):
    """A population of random walks over a graph: node_keys (a list per walk), n_steps, and every step's parameters on the device
    (`parameters`, a _capi.DeviceBuffer of (n_walks, s_max, ld) `dtype`; row (w, i) holds the n_gmm_dims parameters of step i of
    walk w, zeros behind them and for the steps a walk does not have)."""

    def __init__(self, graph, node_keys, seed=0, dtype=np.float64, ctx=None):
        self.graph, self.node_keys, self.seed, self.dtype = graph, [list(keys) for keys in node_keys], int(seed), np.dtype(dtype)
        self.nodes, self.node_of, self.n_steps = walk_tables(self.node_keys, graph.nodes)
        self._mps = [_primitive_of(graph.nodes[key]) for key in self.nodes]
        self._prims = [mp._prim for mp in self._mps]
        self.ctx = ctx or self._prims[0].ctx
        self.ld = max(p.n_gmm_dims for p in self._prims)
        self.parameters = self.ctx.malloc(self.node_of.size * self.ld * self.dtype.itemsize)
        self.components = self.ctx.malloc(self.node_of.size * 4)
        sample_walk_latents_dev(self._prims, self.node_of, self.n_steps, self.seed, self.parameters, self.dtype, self.ld, self.components)

    @property
    def n_walks(self):
        return len(self.node_keys)

    def parameters_host(self):
        """(n_walks, s_max, ld) of the population's dtype."""
        return self.ctx.download(self.parameters, self.node_of.shape + (self.ld,), self.dtype)

    def components_host(self):
        """(n_walks, s_max) int32: the mixture component every step was drawn from, -1 for the steps a walk does not have."""
        return self.ctx.download(self.components, self.node_of.shape, np.int32)

    def frame_offsets(self, lengths=None):
        """(n_walks, s_max + 1) int64: the first row of every step inside its walk, back to back; [w, n_steps[w]:] is the walk's length.
        lengths: None (the canonical grids) or (n_walks, s_max), the samples of every step's time row (time_functions)."""
        if lengths is None:
            T = np.array([mp.n_canonical_frames for mp in self._mps], dtype=np.int64)
            lengths = T[np.maximum(self.node_of, 0)]
        lengths = np.where(self.node_of >= 0, np.asarray(lengths, dtype=np.int64), 0)
        offsets = np.zeros((self.n_walks, self.node_of.shape[1] + 1), dtype=np.int64)
        offsets[:, 1:] = np.cumsum(lengths, axis=1)
        return offsets

    def time_functions(self, speed=1.0):
        """Every step's time row from ONE mg_walks_time_functions launch and one download of the lengths: (d_times, a device
        buffer of (n_walks, s_max, t_cap) float64, the caller's to free, lengths int32 (n_walks, s_max), 0 for the steps a walk
        does not have, t_cap).  t_cap starts by graph_walk._sample_times' rule; a row that needs more reports how
        many and the table is laid out again.  ValueError for a time function that is not finite.  smooth_time_parameters on a
        node's primitive is refused -- unless the primitive opts in with smooth_on_device: then ONE
        mg_walks_time_functions_smoothed launch smooths those nodes' rows on their way out, and a row of fewer than 15 samples
        raises ValueError naming its (walk, step), as scipy would, before any frames launch."""
        from .time_smoothing import require_smoothing_window
        has_time = [mp.has_time_parameters and mp.get_n_time_components() > 0 for mp in self._mps]
        smooths = [bool(ht and mp.smooth_time_parameters) for mp, ht in zip(self._mps, has_time)]
        if any(sm and not getattr(mp, "smooth_on_device", False) for mp, sm in zip(self._mps, smooths)):
            raise NotImplementedError("smoothed time functions (smooth_time_parameters): set smooth_on_device on the primitive for the Savitzky-Golay pass "
                                      "inside the time kernel")
        t_cap = max(int(4 * mp.n_canonical_frames / min(float(speed), 1.0)) + 8 if ht else len(_untimed_grid(mp.n_canonical_frames, speed))
                    for mp, ht in zip(self._mps, has_time))
        with self.ctx.buffers() as own:
            d_l = own.malloc(4 * self.node_of.size)
            while True:
                d_t = own.malloc(8 * self.node_of.size * t_cap)
                if any(smooths):
                    walks_time_functions_smoothed_dev(self._prims, self.node_of, self.n_steps, smooths, self.parameters, self.dtype, self.ld, speed, d_t, d_l, t_cap)
                else:
                    walks_time_functions_dev(self._prims, self.node_of, self.n_steps, self.parameters, self.dtype, self.ld, speed, d_t, d_l, t_cap)
                lengths = self.ctx.download(d_l, self.node_of.shape, np.int32)
                if ((lengths == 0) & (self.node_of >= 0)).any():
                    raise ValueError("a time function is not finite")
                if lengths.min() >= 0:
                    if any(smooths):
                        require_smoothing_window(np.where(np.array(smooths)[np.maximum(self.node_of, 0)] & (self.node_of >= 0), lengths, 0), "walk %d, step %d")
                    return own.release(d_t), lengths, t_cap
                t_cap = int(-lengths.min()) + 8              # (negative: the samples the row would need)

    def frames(self, alignment=None, skeleton=None, with_transforms=False, use_time_parameters=False, speed=1.0):
        """Every walk's motion from ONE mg_walks_frames call: a list of (T_w, n_dim) float64 arrays (views of one download);
        alignment: of every walk's first step (None, a previous-frame record, a start-pose record), skeleton as in
        graph_walk.assemble_walks.  with_transforms: also (n_walks, s_max, 4) = (c, s, tx, tz), NaN for the steps a walk does
        not have.  use_time_parameters: the time-warped motion at `speed` -- one mg_walks_time_functions launch, the download of
        the lengths, one mg_walks_frames_at call; every T_w is that walk's own."""
        if not use_time_parameters and float(speed) != 1.0:
            raise NotImplementedError("a speed other than 1 on the canonical grid")
        n, s_max, D = self.n_walks, self.node_of.shape[1], self._prims[0].n_dim
        with self.ctx.buffers() as bufs:
            if use_time_parameters:
                d_t, lengths, t_cap = self.time_functions(speed)
                bufs.bufs.append(d_t)                        # (freed with the call's other buffers)
                offsets = self.frame_offsets(lengths)
            else:
                offsets = self.frame_offsets()
            stride = int(offsets[:, -1].max())
            d_f = bufs.malloc(8 * n * stride * D)
            d_x = bufs.upload(np.full((n, s_max, 4), np.nan)) if with_transforms else None
            if use_time_parameters:
                walks_frames_at_dev(self._prims, self.node_of, self.n_steps, self.parameters, self.dtype, self.ld, d_t, lengths, t_cap, offsets[:, :-1], d_f, stride,
                                    alignment, skeleton, d_x)
            else:
                walks_frames_dev(self._prims, self.node_of, self.n_steps, self.parameters, self.dtype, self.ld, d_f, stride, None, alignment, skeleton, d_x)
            block = self.ctx.download(d_f, (n, stride, D), np.float64)
            transforms = self.ctx.download(d_x, (n, s_max, 4), np.float64) if with_transforms else None
        frames = [block[w, :int(offsets[w, -1])] for w in range(n)]
        return (frames, transforms) if with_transforms else frames

    def to_graph_walks(self, skeleton=None, use_time_parameters=False):
        """A HipGraphWalk per walk with its steps filled (node key, the step's n_gmm_dims parameters as float64), for the
        optimiser and the JSON export."""
        params = self.parameters_host()
        walks = []
        for w, keys in enumerate(self.node_keys):
            walk = HipGraphWalk(self.graph, use_time_parameters=use_time_parameters, skeleton=skeleton, ctx=self.ctx)
            for i, key in enumerate(keys):
                width = self._prims[self.node_of[w, i]].n_gmm_dims
                walk.steps.append(HipGraphWalkStep.from_graph(self.graph, tuple(key), params[w, i, :width]))
            walks.append(walk)
        return walks

    def to_entries(self):
        """The reference's return value per walk: a list of {"node_key", "parameters"}."""
        params = self.parameters_host()
        return [[{"node_key": key, "parameters": np.array(params[w, i, :self._prims[self.node_of[w, i]].n_gmm_dims], dtype=np.float64)}
                 for i, key in enumerate(keys)] for w, keys in enumerate(self.node_keys)]

    def close(self):
        for buf in (self.parameters, self.components):
            if buf is not None:
                buf.free()
        self.parameters = self.components = None


def generate_random_walks(graph, start_action, number_of_steps, n_walks, seed, rng=None, dtype=np.float64):
    """HipMotionStateGraph.generate_random_walks."""
    return RandomWalks(graph, choose_random_walks(graph, start_action, number_of_steps, n_walks, rng), seed, dtype)


def generate_random_walk(graph, start_action, number_of_steps, use_transition_model=True):
    """HipMotionStateGraph.generate_random_walk.  With transition models on the action's edges and use_transition_model the
    reference predicts a step's parameters from the step before it; the predictor class is not in the reference tree:
    NotImplementedError, before anything is drawn.  Without them it samples from the node, as here."""
    if start_action not in graph.node_groups:
        raise KeyError("the graph has no action %r" % (start_action,))
    if use_transition_model and has_transition_models(graph, start_action):
        raise NotImplementedError("parameters predicted by transition models (use_transition_model=False samples from the nodes)")
    node_keys = choose_random_walks(graph, start_action, number_of_steps, 1)
    walks = RandomWalks(graph, node_keys, int(np.random.randint(0, 2 ** 31 - 1)))
    try:
        return walks.to_entries()[0]
    finally:
        walks.close()
