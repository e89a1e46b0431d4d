"""The likelihood contract of include/poco_hip.h (poco_flow_context, poco_flow_nll, poco_flow_nll_reduce,
poco_evaluator_uncert_summary) restated in numpy: the yardstick of tests/test_likelihood_*.py and the host path
tools/bench_eval.py --likelihood times.  dtype = np.float32 mirrors the reference, np.float64 is the yardstick.  Each function
cites the reference lines it restates; none of their text is copied.

    context            nf_head.py:82
    residual           nf_head.py:89-105 (batch_rodrigues: tests/eval_np.rodrigues)
    log_prob           real_nvp.py:40-65 through oracle/poco_ref.realnvp_log_prob, nf_head.py:106-112
    flow_nll, summary  nf_head.py:84-123, losses.py:346 (nf_loss_weight = 1)
    uncert_summary     trainer.py:374,377-378 with poco_utils.py:151-169,265-281
"""
import numpy as np
import torch

from oracle import poco_ref
from tests import eval_np, util

RECORD_FLOATS = 80
N_VALID, N_SUM, N_LOGPHI, N_LOGSIGMA, N_BAR = 0, 1, 8, 32, 56        # record offsets (include/poco_hip.h)


def flow_weights(variant, seed=0):
    """The flow_head.* tensors of util.synth_weights(variant, seed) (tensors are keyed by name: the same values)."""
    from poco_amd import synth
    spec = [(n, s) for n, s in util.load_spec(variant) if n.startswith("flow_head.")]
    return synth.synth_state_dict(spec, seed)


def context(w, uncert_feat, dtype=np.float64):
    """uncert_feat [B,in_ctx] -> [B,512]."""
    W, b = np.asarray(w["flow_head.cond_layer.weight"], dtype), np.asarray(w["flow_head.cond_layer.bias"], dtype)
    return np.asarray(uncert_feat, dtype) @ W.T + b


def residual(pred_pose, gt_pose, var_pose, dtype=np.float64):
    """-> bar [B,24,3,3]; its reshape(-1, 9) are the rows the flow sees."""
    g = eval_np.rodrigues(np.asarray(gt_pose).reshape(-1, 3), dtype).reshape(-1, 24, 3, 3)
    sigma = np.asarray(var_pose, dtype)[:, :, None, None]
    return np.abs(np.asarray(pred_pose, dtype) - g) / (sigma + dtype(1e-9))


def log_prob(w, rows, ctx, dtype=np.float64):
    """rows [B*24,9], ctx [B,512] (repeated over the 24 rows of a crop here) -> [B,24]."""
    tt = torch.float64 if dtype == np.float64 else torch.float32
    sd = {k: torch.from_numpy(np.asarray(v)).to(tt) for k, v in w.items() if k.startswith("flow_head.flow.")}
    x = torch.from_numpy(np.ascontiguousarray(rows, dtype))
    c = torch.from_numpy(np.repeat(np.ascontiguousarray(ctx, dtype), 24, axis=0))
    with torch.no_grad():
        return poco_ref.realnvp_log_prob(sd, x, c).numpy().reshape(-1, 24)


def flow_nll(w, pred_pose, gt_pose, var_pose, ctx, valid=None, dtype=np.float64):
    """Everything poco_flow_nll computes for B crops as a dict: bar_rows [B*24,9], bar_pose / log_phi / log_sigma [B,24], sum [B],
    valid [B].  Invalid crops are computed too; records() zeroes them, summary() leaves them out."""
    B = len(pred_pose)
    bar = residual(pred_pose, gt_pose, var_pose, dtype)
    rows = bar.reshape(-1, 9)
    lp = log_prob(w, rows, ctx, dtype)
    ls = np.log(np.asarray(var_pose, dtype))
    v = np.ones(B, bool) if valid is None else np.asarray(valid).astype(bool)
    return {"bar_rows": rows, "bar_pose": bar.reshape(B, 24, 9).mean(-1), "log_phi": lp, "log_sigma": ls, "sum": (ls - lp).sum(1), "valid": v}


def records(y):
    """flow_nll() -> [B,80] in the record layout (float64: compare, do not expect bits)."""
    B = len(y["valid"])
    rec = np.zeros((B, RECORD_FLOATS), np.float64)
    rec[:, N_VALID] = 1.0
    rec[:, N_SUM] = y["sum"]
    rec[:, N_LOGPHI:N_LOGPHI + 24] = y["log_phi"]
    rec[:, N_LOGSIGMA:N_LOGSIGMA + 24] = y["log_sigma"]
    rec[:, N_BAR:N_BAR + 24] = y["bar_pose"]
    rec[~y["valid"]] = 0.0
    return rec


def summary(rec):
    """[N,80] records -> (valid crops, mean log phi, mean log sigma, loss_nf), float64; NaN means without a valid crop."""
    rec = np.asarray(rec, np.float64)
    v = rec[:, N_VALID] != 0
    lp, ls = rec[v, N_LOGPHI:N_LOGPHI + 24], rec[v, N_LOGSIGMA:N_LOGSIGMA + 24]
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.float64(24 * v.sum())
        return int(v.sum()), lp.sum() / n, ls.sum() / n, (ls - lp).sum() / n


def uncert_summary(eval_records):
    """The evaluator's [N,416] records -> (Var-MPJPE, Variance), float64, metres."""
    rec = np.asarray(eval_records, np.float64)
    u = rec[:, eval_np.R_UNC:eval_np.R_UNC + 24].mean(1)
    return float((rec[:, eval_np.R_MPJPE] / (u + 1e-9)).mean()), float(u.mean())


FIXTURE_CROPS = 16
FIXTURE_INVALID = (3, 11)                       # has_smpl = 0
CTX_KEEP = 4                                    # the fixture stores every 4th column of the [16,512] context (file size)
FIXTURE_CASES = [("resnet50-cliff", 1, 2048), ("hrnet_w32-pare", 3, 3072)]     # (variant, NUM_FLOW_LAYERS, in_ctx): both depths, both widths


def case_tag(variant):
    return variant.split("-")[1]


def fixture_inputs(variant, seed: int = 4242):
    """The inputs tests/golden/likelihood.npz was made from, re-derived from seeds (the file stores only expected outputs):
    uncert_feat ~ N(0, 1); axis-angle ground truth with angles up to pi; the prediction a 0.1 rad perturbation of it; sigma drawn
    from [0.05, 0.55]; has_smpl = 0 for FIXTURE_INVALID.  float32, as the engine's tensors."""
    in_ctx = {v: c for v, _, c in FIXTURE_CASES}[variant]
    r = np.random.default_rng([seed, in_ctx])
    B = FIXTURE_CROPS
    uf = r.standard_normal((B, in_ctx)).astype(np.float32)
    ax = r.standard_normal((B, 24, 3))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    gt_pose = (ax * r.uniform(0.0, np.pi, (B, 24, 1))).reshape(B, 72).astype(np.float32)
    pert = gt_pose.astype(np.float64) + 0.1 * r.standard_normal((B, 72))
    pred_pose = eval_np.rodrigues(pert.reshape(-1, 3), np.float64).reshape(B, 24, 3, 3).astype(np.float32)
    var_pose = r.uniform(0.05, 0.55, (B, 24)).astype(np.float32)
    has_smpl = np.ones(B, np.int32)
    has_smpl[list(FIXTURE_INVALID)] = 0
    return {"uncert_feat": uf, "gt_pose": gt_pose, "pred_pose": pred_pose, "var_pose": var_pose, "has_smpl": has_smpl}
