"""Make tests/golden/pseudo.npz: the outputs of the REFERENCE's own functions on the seeded inputs of tests/pseudo_np.py.  CPU
only; needs the reference checkout (oracle/ref_import.py).

    python tools/gen_pseudo_golden.py

Runs rotation_matrix_to_angle_axis and batch_rodrigues (pocolib/utils/geometry.py), get_confident_frames
(pocolib/utils/train_utils.py) and get_kinematic_uncert (pocolib/utils/poco_utils.py) and stores ONLY data: the float32 inputs
(`rotmat`, their class `cls`, `var`, `threshold`), the reference's float32 outputs (`aa`, `rod_of_aa`, `var_kinematic`,
`confident_idx`) and `d_ref_aa` / `d_ref_roundtrip`: the largest deviation of the reference's float32 axis-angle, and of its
batch_rodrigues(aa) - R, from tests/pseudo_np.py in float64 on the same float32 inputs - the unit of every tolerance in
tests/test_pseudo_*.py.  Asserts that all four quaternion branches occur, among the dedicated `branch` rows and overall, and that
no component changes sign between the float32 and the float64 evaluation."""
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import ref_import  # noqa: E402
from poco_amd import synth  # noqa: E402
from tests import pseudo_np  # noqa: E402

OUT = ROOT / "tests" / "golden" / "pseudo.npz"


def main():
    assert ref_import.available(), "needs the reference checkout"
    torch.set_num_threads(8)
    mp = synth.synth_state_dict([("head.init_pose", (1, 144)), ("head.init_shape", (1, 10)), ("head.init_cam", (1, 3))], 0)
    ref_import.setup({"pose": mp["head.init_pose"][0], "shape": mp["head.init_shape"][0], "cam": mp["head.init_cam"][0]})
    hu = ref_import.setup_host_utils()
    geo = importlib.import_module("pocolib.utils.geometry")
    tu = importlib.import_module("pocolib.utils.train_utils")
    assert geo.__file__.startswith(ref_import.REFERENCE) and tu.__file__.startswith(ref_import.REFERENCE)

    R, cls = pseudo_np.fixture_matrices()
    branch = pseudo_np.quaternion_branch(R)
    assert sorted(set(branch.tolist())) == [0, 1, 2, 3], np.bincount(branch)
    assert sorted(branch[cls == pseudo_np.CLASSES.index("branch")].tolist()) == [0, 1, 2, 3]
    aa = geo.rotation_matrix_to_angle_axis(torch.from_numpy(R.copy())).numpy()
    aa64 = pseudo_np.rotmat_to_aa(R, np.float64)
    d_aa = float(np.abs(aa.astype(np.float64) - aa64.astype(np.float64)).max())
    big = np.abs(aa64) > 1e-3
    assert np.array_equal(np.sign(aa)[big], np.sign(aa64)[big]), "a component changed sign between float32 and float64"
    special = np.isin(cls, [pseudo_np.CLASSES.index(c) for c in ("zero", "nan")])
    rod = geo.batch_rodrigues(torch.from_numpy(aa.copy())).numpy()
    rod64 = pseudo_np.rodrigues(aa64, np.float64)
    d_rt = float(np.abs((rod[~special].astype(np.float64) - R[~special]) - (rod64[~special] - R[~special])).max())

    var = pseudo_np.fixture_var()
    thr = pseudo_np.FIXTURE_THRESHOLD
    idx = np.asarray(tu.get_confident_frames(var.copy(), thr), np.int64)
    kin = hu["poco_utils"].get_kinematic_uncert(var.copy())
    assert 9 not in idx and 5 not in idx and 0 < len(idx) < len(var)
    assert d_aa > 0.0 and d_rt > 0.0
    o = {"rotmat": R, "cls": cls, "aa": aa.astype(np.float32), "rod_of_aa": rod.astype(np.float32), "var": var,
         "threshold": np.float64(thr), "confident_idx": idx, "var_kinematic": np.asarray(kin, np.float32),
         "d_ref_aa": np.float64(d_aa), "d_ref_roundtrip": np.float64(d_rt)}
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **o)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): {len(R)} matrices, branches {np.bincount(branch).tolist()}, "
          f"{len(idx)} of {len(var)} rows confident")
    print(f"  d_ref_aa = {d_aa:.3e}\n  d_ref_roundtrip = {d_rt:.3e}")


if __name__ == "__main__":
    main()
