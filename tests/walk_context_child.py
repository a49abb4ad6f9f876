"""Child process of tests/test_gpu_graph_walk_context.py: mg_joint_tracks and mg_walk_frames on ONE context, both with more
dynamic LDS than a kernel gets without its attribute (64 KiB), in the order given on the command line.  The attribute is set
once per process and device, so each order needs a process that has launched neither kernel.
usage: python walk_context_child.py tracks-first|walk-first"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from morphablegraphs_amd import _capi, synthetic  # noqa: E402
from morphablegraphs_amd import graph_walk as gw  # noqa: E402
from morphablegraphs_amd.motion_state_graph import HipPrimitiveSet  # noqa: E402

N_BASIS, D, L, F = 104, 79, 3, 40        # 104 x 79 control-point rows: 66 KiB in mg_walk_frames_kernel, 103 KiB in mg_joint_tracks_kernel


def main(order):
    data = synthetic.make_primitive(seed=31, n_components=L, n_frames=F, n_basis=N_BASIS, n_dim=D, n_gmm=2, name="big")
    mp = HipPrimitiveSet([data], context=_capi.Context(0)).nodes["big"]
    prim, ctx = mp._prim, mp._prim.ctx
    joints, animated = synthetic.make_skeleton(19)
    sk = _capi.Skeleton(joints, animated)
    S = 0.7 * np.random.default_rng(1).standard_normal((2, L))

    def tracks():
        plan = _capi.TrackPlan(prim, sk, [["LeftHand"]], align_joint=0)
        with ctx.buffers() as bufs:
            d_S, d_o = bufs.upload(S), bufs.malloc(2 * F * 3 * 8)
            plan.tracks_dev(d_S, S.dtype, 2, L, [None], [d_o])
            got = ctx.download(d_o, (2, F, 1, 3), np.float64)
        plan.close()
        ref = prim.joint_tracks(sk, ["LeftHand"], S)
        # float64 on both sides, positions of the order of 100 behind a chain of seven joints: 1e-9 is far above the rounding
        assert np.max(np.abs(got - ref)) <= 1e-9, np.max(np.abs(got - ref))

    def walk():
        with ctx.buffers() as bufs:
            d_S, d_f = bufs.upload(S), bufs.malloc(2 * F * D * 8)
            gw.walk_frames_dev([prim], [0], d_S, S.dtype, 2, L, d_f, F)
            got = ctx.download(d_f, (2, F, D), np.float64)
        assert np.array_equal(got, prim.back_project_frames_f64(S))

    for step in ((tracks, walk) if order == "tracks-first" else (walk, tracks)):
        step()
    ctx.synchronize()
    print("ok", order)


if __name__ == "__main__":
    main(sys.argv[1])
