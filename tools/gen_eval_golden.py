"""Make tests/golden/eval.npz: the evaluation metrics of the REFERENCE's own functions on the seeded inputs of
tests/eval_np.fixture_inputs.  CPU only; needs the reference checkout (oracle/ref_import.py) and scipy.

    python tools/gen_eval_golden.py

Runs get_jnts_from_mesh, mpjpe_error, pampjpe_error, vert_error, calculate_distance_pose, calculate_pearson_coff
(pocolib/utils/eval_utils.py), batch_rodrigues (pocolib/utils/geometry.py) and POCOUtils.prepare_uncert
(pocolib/utils/poco_utils.py) and stores ONLY their outputs (numeric arrays) plus `d_ref_<quantity>`: the largest deviation of
those float32 results from tests/eval_np.py in float64 on the same inputs - the unit of every tolerance in tests/test_eval_*.py.
Asserts that every crop is well conditioned ((sigma2 - sigma3) / sigma1 of K above 0.05) and that the mirrored crops are
mirrored (det(U V^T) < 0), so no case has to be left out of any comparison."""
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import ref_import  # noqa: E402
from poco_amd import synth  # noqa: E402
from tests import eval_np  # noqa: E402

OUT = ROOT / "tests" / "golden" / "eval.npz"


def main():
    assert ref_import.available(), "needs the reference checkout"
    torch.set_num_threads(8)
    mp = synth.synth_state_dict([("head.init_pose", (1, 144)), ("head.init_shape", (1, 10)), ("head.init_cam", (1, 3))], 0)
    ref_import.setup({"pose": mp["head.init_pose"][0], "shape": mp["head.init_shape"][0], "cam": mp["head.init_cam"][0]})
    hu = ref_import.setup_host_utils()
    eu = importlib.import_module("pocolib.utils.eval_utils")
    geo = importlib.import_module("pocolib.utils.geometry")
    assert eu.__file__.startswith(ref_import.REFERENCE)

    inp = eval_np.fixture_inputs()
    t = torch.from_numpy
    J = t(inp["J_regressor"])
    o, dref = {}, {}

    def dev(q, a, b):
        dref[q] = max(dref.get(q, 0.0), float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()))

    ratios, dets = [], []
    for form, name in eval_np.FIXTURE_COMBOS:
        jm = eval_np.joint_map(name)
        tag = f"{form}_{len(jm)}"
        pj, pj_nonrel = eu.get_jnts_from_mesh(t(inp["pred_vertices"]), J, name)
        if form == "verts":
            gj = eu.get_jnts_from_mesh(t(inp["gt_vertices"]), J, name)[0]          # base_dataset.py:359-365: the same arithmetic
            v2v = eu.vert_error(t(inp["pred_vertices"]), t(inp["gt_vertices"]))
        else:
            gj = t(inp["gt_joints"][name])
            v2v = eu.vert_error(t(inp["pred_vertices"]), None)
        _, e = eu.mpjpe_error(pj, gj)
        _, r = eu.pampjpe_error(pj, gj, reduction=None)
        ref = {"mpjpe": e, "pampjpe": r, "v2v": np.asarray(v2v, np.float32), "pred_jnts3D": pj.numpy(), "gt_jnts3D": gj.numpy(),
               "pred_jnts3D_nonrel": pj_nonrel.numpy()}
        y64 = eval_np.evaluate(**eval_np.fixture_case(inp, form, name), dtype=np.float64)
        for k, v in ref.items():
            o[f"{tag}_{k}"] = np.asarray(v, np.float32)
            dev("joints" if "jnts" in k else k, v, y64[k])
        for b in range(eval_np.FIXTURE_CROPS):
            ratio, det = eval_np.conditioning(y64["pred_jnts3D"][b], y64["gt_jnts3D"][b])
            ratios.append(ratio)
            dets.append(det)
            assert ratio > 0.05, (tag, b, ratio)
            assert (det < 0) == (b in eval_np.FIXTURE_MIRRORED), (tag, b, det)
    # correlation inputs: the same for every combination
    cx = eu.calculate_distance_pose(t(inp["pred_pose"]), t(inp["gt_pose"])).numpy()
    o["corr_x"] = cx
    dev("corr_x", cx, eval_np.pose_distance(inp["pred_pose"], inp["gt_pose"], np.float64))
    for kin in (True, False):
        pu = ref_import.poco_utils_instance(hu, "hrnet_w48_cls-cliff", kin)
        cy = np.asarray(pu.prepare_uncert(t(inp["var_pose"].copy())), np.float32)
        o["corr_y_kin" if kin else "corr_y_nokin"] = cy
        dev("corr_y", cy, eval_np.processed_uncert(inp["var_pose"], kin, np.float64))
    rr, _ = eu.calculate_pearson_coff(o["corr_x"].flatten().astype(np.float64), o["corr_y_kin"].flatten().astype(np.float64))
    o["pearson"] = np.asarray(rr, np.float64)
    rod = geo.batch_rodrigues(t(inp["rod_aa"])).numpy()
    o["rodrigues"] = rod
    dev("rodrigues", rod, eval_np.rodrigues(inp["rod_aa"], np.float64))
    for q, v in dref.items():
        assert v > 0.0, q
        o[f"d_ref_{q}"] = np.float64(v)
    o["min_sigma_ratio"] = np.float64(min(ratios))
    o["dets"] = np.asarray(dets, np.float64)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **o)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes); min (s2 - s3) / s1 = {min(ratios):.3f}")
    for q, v in sorted(dref.items()):
        print(f"  d_ref_{q} = {v:.3e}")


if __name__ == "__main__":
    main()
