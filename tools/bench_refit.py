"""Time the keypoint refit (poco_amd/refit.py, csrc/kp_refit.hip), after warm-up:

    python tools/bench_refit.py [--iters 20] [--out profiles/refit_step.txt]

  (a) the operator alone (one launch), device events around the Python call, at 1 / 8 tracks x 300 / 3000 frames, LAMBDA 0.1,
      10 steps, 25 keypoints of which 14 are mapped;
  (b) the whole step on the same tracks (not at 8 x 3000, whose meshes are 2 GB on the host), wall clock: refit_tracks = upload,
      the rest joints' matmul, the operator, LBS of every fitted row, download;
  (c) the host form it stands in for, wall clock: tests/refit_np.py in float64 on 24 rows, scaled to the buffer's rows.
Video mode with and without --kp_refit is not timed here.  Prints one line per measurement; --out also writes them to a file.  No
pass / fail ratio."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import refit, synth  # noqa: E402
from tests import refit_np as rn, util  # noqa: E402
from tools.bench_eval import event_ms  # noqa: E402
from tools.bench_infill import wall_ms  # noqa: E402

LAM = 0.1
W, H = 1280, 720


def make_tracks(P, T, tables, seed):
    """Tracks whose keypoints are the projection of a pose a few degrees from the network's, plus 2 % of the box of noise."""
    r = np.random.default_rng(seed)
    base = rn.gpu_case(N=60, seed=seed)
    good = np.nonzero(np.isfinite(base["pose"]).all((1, 2, 3)) & np.isfinite(base["kp"]).all((1, 2)))[0]
    idx = good[np.arange(T) % len(good)]
    Jt, Jd, _ = tables
    tracks = {}
    for p in range(P):
        betas = (0.5 * r.standard_normal((T, 10))).astype(np.float32)
        pose = base["pose"][idx].copy()
        J = (Jt[None] + np.einsum("jck,nk->njc", Jd, betas.astype(np.float64))).astype(np.float32)
        h = np.full(T, 300.0, np.float32)
        oc = np.stack([np.full(T, 0.9 * 300 / W), np.full(T, 0.9 * 300 / H), r.uniform(-0.1, 0.1, T), r.uniform(-0.1, 0.1, T)], 1).astype(np.float32)
        cam5 = np.stack([oc[:, 0] * np.float32(W / 2), oc[:, 2], oc[:, 3], np.full(T, W / 2), np.full(T, H / 2)], 1).astype(np.float64)
        kp = np.zeros((T, 25, 3), np.float32)
        for t in range(min(T, 60)):                        # 60 distinct rows, repeated: the operator's time does not depend on the data
            turned = np.stack([pose[t, j].astype(np.float64) @ rn.rot_axis(r.standard_normal(3), np.deg2rad(r.uniform(0, 12))) for j in range(24)])
            kp[t, :, :2] = rn.project(turned, J[t], cam5[t]) + r.standard_normal((25, 2)) * 6.0
            kp[t, :, 2] = r.uniform(0.35, 1.0, 25)
        for t in range(60, T):
            kp[t] = kp[t % 60]
            pose[t], betas[t], oc[t] = pose[t % 60], betas[t % 60], oc[t % 60]
        tracks[str(p)] = {"pose": pose, "betas": betas, "orig_cam": oc, "frame_ids": np.arange(T), "joints2d": kp,
                          "bboxes": np.stack([np.full(T, W / 2), np.full(T, H / 2), h, h], 1).astype(np.float32),
                          "var": r.uniform(0.05, 3.0, (T, 24)).astype(np.float32), "verts": np.zeros((T, 6890, 3), np.float32),
                          "smpl_joints3d": np.zeros((T, 49, 3), np.float32)}
    return tracks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_refit.py needs a GPU"
    dev = torch.device("cuda:0")
    model = util.make_engine("resnet50-cliff", max_batch=64)
    tables = refit.joint_tables(synth.synth_smpl(7))
    lines = [f"# keypoint refit on {torch.cuda.get_device_name(0)}: LAMBDA {LAM}, 10 steps, K = 25 (14 mapped); ms = median (min .. max)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for P, T in ((1, 300), (8, 300), (1, 3000), (8, 3000)):
        tracks = make_tracks(P, T, tables, 7 + P + T)
        if P * T > 3000:
            for tr in tracks.values():
                tr["verts"] = tr["smpl_joints3d"] = None
        N = P * T
        cat = lambda k: np.ascontiguousarray(np.concatenate([tracks[str(p)][k] for p in range(P)]), np.float32)   # noqa: E731
        oc = cat("orig_cam")
        cam = np.stack([oc[:, 0] * np.float32(W / 2), oc[:, 2], oc[:, 3], np.full(N, W / 2, np.float32), np.full(N, H / 2, np.float32)], 1)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)                               # noqa: E731
        dp, dv, db, dk, dc, dn = up(cat("pose")), up(cat("var")), up(cat("betas")), up(cat("joints2d")), up(cam), up(cat("bboxes")[:, 2])
        res = refit.refit_rows(tables, dp, dv, db, dk, dc, dn, LAM)
        info = res["info"].cpu().numpy()
        med, lo, hi = event_ms(lambda: refit.refit_rows(tables, dp, dv, db, dk, dc, dn, LAM), a.iters)
        say(f"(a) operator   {P} x {T:4d} rows: {med:8.3f} ms ({lo:.3f} .. {hi:.3f}), {1e3 * med / N:.2f} us per row; "
            f"{int((info[:, 1] == 0).sum())} of {N} fitted, {info[:, 0].mean():.1f} steps accepted on average")
        if N > 3000:                                       # 24000 meshes are 2 GB on the host: the operator's line stands alone
            continue
        med, lo, hi = wall_ms(lambda: refit.refit_tracks(model, tracks, LAM, tables=tables, img_w=W, img_h=H), max(a.iters // 4, 3))
        say(f"(b) whole step {P} x {T:4d} rows: {med:8.3f} ms ({lo:.3f} .. {hi:.3f}) with upload, LBS of every fitted row and download")
        if (P, T) == (1, 300):
            n = 24
            jr = refit.rest_joints(tables, db[:n]).cpu().numpy()
            t0 = time.perf_counter()
            rn.refit(cat("pose")[:n], cat("var")[:n], jr, cat("joints2d")[:n], cam[:n], cat("bboxes")[:n, 2], lam=LAM)
            per_row = 1e3 * (time.perf_counter() - t0) / n
            say(f"(c) numpy restatement (float64, plain loops): {per_row:.2f} ms per row on {n} rows = "
                + ", ".join(f"{per_row * p * t / 1e3:.1f} s for {p} x {t}" for p, t in ((1, 300), (8, 300), (1, 3000), (8, 3000))))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
