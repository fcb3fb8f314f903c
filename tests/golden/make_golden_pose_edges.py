"""Generate tests/golden/golden_pose_edges.npz: the pose tail of tests/golden/pose_edge_inputs.py by the REFERENCE's
own functions (imported read-only through make_golden.import_reference); only data is written.

The statements are those the samplers end in: normalize_rotation(pose[:, :6], 'rot_matrix') (utils/misc.py), then
get_rot_matrix(.., 'rot_matrix') and matrix_to_quaternion (posenet_agent.py pred_func), on torch CPU tensors, once
in float32 and once in float64 (the float32 inputs widened). The file holds the expected outputs and a digest of
the inputs; the inputs are rebuilt from their seed by the tests.

Usage:  python tests/golden/make_golden_pose_edges.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden  # noqa: E402  (sets the paths, imports torch)
import pose_edge_inputs as pe  # noqa: E402
import torch  # noqa: E402


def main():
    make_golden.import_reference("pc", 20)
    from utils.misc import get_rot_matrix, normalize_rotation
    from utils.transforms.rotation_conversions import matrix_to_quaternion
    inp = pe.build()
    out = dict(digest=np.array(pe.digest(inp)))
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        rot6 = torch.from_numpy(inp["rows"][:, :6].copy()).to(dt)
        gs = normalize_rotation(rot6.clone(), "rot_matrix")
        q = matrix_to_quaternion(get_rot_matrix(gs.clone(), "rot_matrix"))
        assert gs.dtype == dt and q.dtype == dt
        out[f"gs_{tag}"], out[f"q_{tag}"] = gs.numpy(), q.numpy()
    path = os.path.join(HERE, "golden_pose_edges.npz")
    np.savez_compressed(path, **out)
    print(f"{len(inp['rows'])} rows -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
