"""mg_walk_frames next to mg_joint_tracks on one context.  Both kernels ask for more than 64 KiB of dynamic LDS on a primitive with
104 x 79 control-point rows, which needs hipFuncAttributeMaxDynamicSharedMemorySize; the library sets it once per context and
remembers that in a bit per kernel family, so the two families must not share a bit.  The attribute itself is kept per process
and device: each order runs in a child process that has launched neither kernel (tests/walk_context_child.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "walk_context_child.py")


@pytest.mark.parametrize("order", ["tracks-first", "walk-first"])
def test_joint_tracks_and_walk_frames_share_a_context(order):
    done = subprocess.run([sys.executable, CHILD, order], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = done.stdout.decode("utf-8", "replace")
    print(out)
    assert done.returncode == 0 and ("ok " + order) in out, out[-2000:]
