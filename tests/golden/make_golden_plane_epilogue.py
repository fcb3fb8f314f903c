"""Records golden_plane_epilogue.npz: the bits the head trunks produced BEFORE the activation-plane epilogues
(gp_head.h split3 / split_act) were rewritten, on an MI355X, from the library of the parent commit.

Run it only with GENPOSE_HIP_LIB pointing at a build of that parent commit (7c847fa); never regenerate the file from
the tree under test: the test that reads it (tests/test_gpu_plane_epilogue.py) exists to show that the rewritten
epilogues changed no bit. Inputs and calls: plane_epilogue_inputs.py (seeded; nothing but seeds and outputs is
stored).

Usage:  GENPOSE_HIP_LIB=/path/to/parent/libgenpose_hip.so python tests/golden/make_golden_plane_epilogue.py [OUT.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import plane_epilogue_inputs as pi  # noqa: E402


def main():
    if "GENPOSE_HIP_LIB" not in os.environ:
        raise SystemExit("set GENPOSE_HIP_LIB to the parent commit's library (see the docstring)")
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "golden_plane_epilogue.npz")
    path, abi = pi.lib_path()
    fix = {"abi_version": np.array([abi], np.int64)}
    for name, a in pi.run_all().items():
        e = pi.entry(a)
        fix[name + "_sha"], fix[name + "_rows"] = e["sha"], e["rows"]
        print(f"{name}: shape {a.shape} {a.dtype}, finite {bool(np.isfinite(a).all())}, sha {e['sha'].tobytes().hex()[:16]}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **fix)
    print(f"wrote {out_path} ({os.path.getsize(out_path)} bytes) from {path} (ABI {abi})")


if __name__ == "__main__":
    main()
