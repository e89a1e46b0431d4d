"""Make tests/golden/likelihood.npz: the flow likelihood of the REFERENCE's own modules on the seeded inputs of
tests/likelihood_np.fixture_inputs.  CPU only; needs the reference checkout (oracle/ref_import.py).

    python tools/gen_likelihood_golden.py

Runs flow_head.forward with `is_train` in the batch (pocolib/models/head/nf_head.py:78-136: cond_layer, batch_rodrigues, the
residual, RealNVP.log_prob), batch_rodrigues (pocolib/utils/geometry.py) and POCOUtils.prepare_uncert (pocolib/utils/poco_utils.py)
for both flow depths and both context widths of the shipped configs, and stores ONLY their outputs (numeric arrays) plus
`d_ref_<quantity>`: the largest deviation of those float32 results from tests/likelihood_np.py in float64 on the same inputs - the
unit of the tolerances in tests/test_likelihood_*.py.  Three one-line formulas whose enclosing functions build torch.cuda tensors and
cannot run on a CPU are restated here on the reference's outputs: nf_head.py:101 (the residual, which forward does not return),
losses.py:346 (loss_nf) and trainer.py:374,377-378 (Var-MPJPE, Variance).
Asserts that the fixture cannot pass vacuously: log_phi differs between crops, and changes when the context rows are permuted, by
more than 100 x its tolerance - a kernel that ignores the residual or the context fails."""
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import ref_import  # noqa: E402
from poco_amd import synth  # noqa: E402
from tests import eval_np, likelihood_np as lnp  # noqa: E402

OUT = ROOT / "tests" / "golden" / "likelihood.npz"


def log_phi_tol(lp):
    """The rule tests/test_model_gpu.py::test_realnvp_op applies to the same kernel."""
    return 1e-3 * max(1.0, float(np.abs(lp).max()))


def main():
    assert ref_import.available(), "needs the reference checkout"
    torch.set_num_threads(8)
    mp = synth.synth_state_dict([("head.init_pose", (1, 144)), ("head.init_shape", (1, 10)), ("head.init_cam", (1, 3))], 0)
    ref_import.setup({"pose": mp["head.init_pose"][0], "shape": mp["head.init_shape"][0], "cam": mp["head.init_cam"][0]})
    hu = ref_import.setup_host_utils()
    nf = importlib.import_module("pocolib.models.head.nf_head")
    geo = importlib.import_module("pocolib.utils.geometry")
    assert nf.__file__.startswith(ref_import.REFERENCE)
    t = torch.from_numpy
    o, dref = {}, {}

    def dev(q, a, b):
        dref[q] = max(dref.get(q, 0.0), float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()))

    for variant, L, in_ctx in lnp.FIXTURE_CASES:
        tag = lnp.case_tag(variant)
        w = lnp.flow_weights(variant)
        fh = nf.flow_head("pose", L, "", "alter", [], 9, True, in_ctx, 512).eval()
        fh.load_state_dict({k[len("flow_head."):]: t(v) for k, v in w.items()}, strict=True)
        inp = lnp.fixture_inputs(variant)
        valid = inp["has_smpl"].astype(bool)
        assert (~valid).sum() >= 2 and inp["var_pose"].min() >= 0.05 and inp["var_pose"].max() <= 0.55

        def forward(uncert_feat):
            pred = {"smpl_vertices": torch.zeros(lnp.FIXTURE_CROPS, 1, 3), "pred_pose": t(inp["pred_pose"]), "var_pose": t(inp["var_pose"])}
            batch = {"is_train": True, "has_smpl": t(inp["has_smpl"]), "pose": t(inp["gt_pose"])}
            with torch.no_grad():
                return fh({"uncert_feat": t(uncert_feat)}, pred, batch)["log_phi"].numpy()

        with torch.no_grad():
            ctx = fh.cond_layer(t(inp["uncert_feat"])).numpy()
            gt_rot = geo.batch_rodrigues(t(inp["gt_pose"]).view(-1, 3)).view(-1, 24, 3, 3)
            sigma = t(inp["var_pose"]).unsqueeze(-1).unsqueeze(-1).repeat(1, 1, 3, 3)
            bar = (torch.abs(t(inp["pred_pose"]) - gt_rot) / (sigma + 1e-9))[t(valid)].reshape(-1, 9).numpy()      # nf_head.py:101,105
            log_sigma = torch.log(t(inp["var_pose"])[t(valid)])
        log_phi = forward(inp["uncert_feat"])
        assert log_phi.shape == (int(valid.sum()), 24) and log_phi.dtype == np.float32
        with torch.no_grad():
            diff = log_sigma - t(log_phi)
            loss_nf = diff.mean().numpy()                                                                            # losses.py:346, weight 1
        ref = {"ctx": ctx, "bar": bar, "log_phi": log_phi, "log_sigma": log_sigma.numpy(), "sum": diff.sum(1).numpy(),
               "mean": np.array([log_phi.mean(), log_sigma.numpy().mean(), loss_nf], np.float32)}
        c64 = lnp.context(w, inp["uncert_feat"], np.float64)
        y64 = lnp.flow_nll(w, inp["pred_pose"], inp["gt_pose"], inp["var_pose"], c64, inp["has_smpl"], np.float64)
        want = {"ctx": c64, "bar": y64["bar_rows"].reshape(-1, 24, 9)[valid].reshape(-1, 9), "log_phi": y64["log_phi"][valid],
                "log_sigma": y64["log_sigma"][valid], "sum": y64["sum"][valid], "mean": np.array(lnp.summary(lnp.records(y64))[1:])}
        for k, v in ref.items():
            o[f"{tag}_{k}"] = np.asarray(v, np.float32)[:, ::lnp.CTX_KEEP] if k == "ctx" else np.asarray(v, np.float32)
            dev(k, v, want[k])                          # (the deviation is taken over every column; every CTX_KEEP-th one is stored)
        # not vacuous: the crops differ, and the context matters, by more than 100 x the tolerance log_phi is held to
        tol = log_phi_tol(log_phi)
        spread = float(np.ptp(log_phi.mean(1)))
        moved = float(np.abs(forward(np.roll(inp["uncert_feat"], 1, axis=0)) - log_phi).max())
        print(f"{tag}: log_phi in [{log_phi.min():.2f}, {log_phi.max():.2f}], tolerance {tol:.2e}, spread over crops {spread:.2f}, "
              f"moved by a permuted context {moved:.2f}, loss_nf {float(loss_nf):.4f}")
        assert spread > 100 * tol and moved > 100 * tol, (tag, spread, moved, tol)
        o[f"{tag}_spread"] = np.float64(spread)
        o[f"{tag}_moved"] = np.float64(moved)
    # Var-MPJPE and Variance: prepare_uncert on the cliff case's sigma, a seeded per-crop MPJPE (metres)
    inp = lnp.fixture_inputs(lnp.FIXTURE_CASES[0][0])
    mpjpe = np.random.default_rng(77).uniform(0.03, 0.15, lnp.FIXTURE_CROPS).astype(np.float32)
    pu = ref_import.poco_utils_instance(hu, "hrnet_w48_cls-cliff", True)
    val_var = np.array(np.asarray(pu.prepare_uncert(t(inp["var_pose"].copy()))).mean(1).tolist())                   # poco_utils.py:169
    val_mpjpe = np.array(mpjpe.tolist())
    o["uncert_summary"] = np.array([(val_mpjpe / (val_var + 1e-9)).mean(), val_var.mean()], np.float64)              # trainer.py:374,377-378
    o["uncert_mpjpe"] = mpjpe
    rec = np.zeros((lnp.FIXTURE_CROPS, eval_np.RECORD_FLOATS), np.float32)
    rec[:, eval_np.R_MPJPE] = mpjpe
    rec[:, eval_np.R_UNC:eval_np.R_UNC + 24] = eval_np.processed_uncert(inp["var_pose"], True, np.float32)
    dev("uncert_summary", o["uncert_summary"], lnp.uncert_summary(rec))
    for q, v in dref.items():
        assert v > 0.0, q
        o[f"d_ref_{q}"] = np.float64(v)
    assert all(v.dtype.kind in "fi" for v in o.values())
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **o)
    assert OUT.stat().st_size <= 100 * 1024, OUT.stat().st_size
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")
    for q, v in sorted(dref.items()):
        print(f"  d_ref_{q} = {v:.3e}")


if __name__ == "__main__":
    main()
