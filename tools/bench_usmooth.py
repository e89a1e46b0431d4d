"""Time video mode's uncertainty-weighted smoother (poco_amd/usmooth.py, csrc/track_smooth.hip), after warm-up:

    python tools/bench_usmooth.py [--iters 30] [--out profiles/usmooth_step.txt]

  (a) the operator alone (one launch), device events around the Python call, at 1 / 8 tracks x 300 / 3000 frames, lambda 10;
  (b) the whole step on the same tracks, wall clock: smooth_tracks = upload of the ragged buffer, the operator, LBS of every row,
      download;
  (c) the host form it stands in for, wall clock: the banded float64 solve in numpy (all 216 + 14 columns of a track at once, the
      factor per joint) + the batched projection of tests/usmooth_np.py + upload of the result;
  (d) one synthetic clip (2 tracks x 150 frames of 96 x 128, resnet50-cliff, batch 64) through POCOTester.run_on_video with and
      without --smooth_uncert, interleaved rounds, and the step's share of the plain run.
Prints one line per measurement; --out also writes them to a file.  No pass / fail ratio."""
import argparse
import statistics
import sys
import tempfile
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import ops, synth, usmooth  # noqa: E402
from tests import infill_np, usmooth_np, util  # noqa: E402
from tools.bench_eval import event_ms  # noqa: E402
from tools.bench_infill import wall_ms  # noqa: E402

LAM, U_REF, GAP = 10.0, 0.3, 30


def make_tracks(P, T, seed):
    r = np.random.default_rng(seed)
    tracks = {}
    for p in range(P):
        R = infill_np.smooth_rotations(r, 64, 2.0)
        tracks[str(p)] = {"pose": np.tile(R, (T // 64 + 1, 1, 1, 1))[:T].copy(), "betas": r.standard_normal((T, 10)).astype(np.float32),
                          "orig_cam": r.standard_normal((T, 4)).astype(np.float32), "frame_ids": np.arange(T),
                          "var": r.uniform(0.05, 3.0, (T, 24)).astype(np.float32), "verts": np.zeros((T, 6890, 3), np.float32),
                          "smpl_joints3d": np.zeros((T, 49, 3), np.float32)}
    return tracks


def host_banded(pose, var, frames, offsets, lin):
    """The restatement's solve done banded in numpy, vectorised over the columns of a joint; then the batched projection."""
    N = pose.shape[0]
    solved, lin64 = np.zeros((N, 24, 9)), np.zeros((N, lin.shape[1]))
    for p in range(len(offsets) - 1):
        lo, hi = int(offsets[p]), int(offsets[p + 1])
        D, om = usmooth_np.penalty(frames[lo:hi], GAP)
        for j in range(24):
            w = usmooth_np.weights(var[lo:hi, j], U_REF)
            Y = pose[lo:hi, j].reshape(hi - lo, 9).astype(np.float64)
            if j == 0:
                Y = np.concatenate([Y, lin[lo:hi].astype(np.float64)], 1)
            X = usmooth_np.solve_banded_ldl(w, D, om, LAM, Y)
            solved[lo:hi, j] = X[:, :9]
            if j == 0:
                lin64[lo:hi] = X[:, 9:]
    return usmooth_np.project_batch(solved.reshape(-1, 3, 3)).reshape(N, 24, 3, 3).astype(np.float32), lin64.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    iters = max(args.iters, 30)
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_usmooth.py on {torch.cuda.get_device_name(0)}, median (min .. max), ms; lambda {LAM:g}, u_ref {U_REF}, "
             f"max_gap {GAP}, u uniform in [0.05, 3]"]
    model = util.make_engine("resnet50-cliff", max_batch=64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    for P, T in ((1, 300), (8, 300), (1, 3000), (8, 3000)):
        tracks = make_tracks(P, T, 100 * P + T)
        cat = lambda k: np.concatenate([tr[k] for tr in tracks.values()])                         # noqa: E731
        pose, var, frames = cat("pose"), cat("var"), cat("frame_ids").astype(np.int32)
        lin = np.concatenate([cat("betas"), cat("orig_cam")], 1)
        offsets = np.arange(P + 1, dtype=np.int32) * T
        dp, du, df, dl, do = t(pose), t(var), t(frames), t(lin), torch.from_numpy(offsets)
        med, lo, hi = event_ms(lambda: ops.track_smooth(dp, du, df, do, dl, LAM, U_REF, GAP), iters)
        lines.append(f"(a) operator {P} x {T}: {med:.4f} ({lo:.4f} .. {hi:.4f})  [one launch + the wrapper's checks and allocations]")
        med, lo, hi = wall_ms(lambda: usmooth.smooth_tracks(model, tracks, LAM, U_REF, GAP), 10 if P * T <= 3000 else 2)
        lines.append(f"(b) step {P} x {T} (all {P * T} rows re-posed): {med:.2f} ({lo:.2f} .. {hi:.2f})")
        if P * T <= 3000:                              # the host form takes seconds per thousand rows: the 24000-row case is left out

            def host():
                ph, lh = host_banded(pose, var, frames, offsets, lin)
                t(ph), t(lh)

            med, lo, hi = wall_ms(host, 1)
            lines.append(f"(c) host form {P} x {T} (banded float64 solve in numpy + projection + upload, no LBS): {med:.1f} ({lo:.1f} .. {hi:.1f})")
    del model
    # (d) video mode with and without the flag
    from poco_amd.tester import POCOTester
    with tempfile.TemporaryDirectory() as tmp:
        w = util.synth_weights("resnet50-cliff")
        torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, f"{tmp}/w.pt")
        np.savez(f"{tmp}/smpl.npz", **synth.synth_smpl(7))
        a = SimpleNamespace(cfg=str(ROOT / "configs" / "demo_poco_cliff_resnet50.yaml"), ckpt=f"{tmp}/w.pt", batch_size=64, smpl=f"{tmp}/smpl.npz",
                            infill=None, smooth=False, smooth_uncert=None, smooth_uncert_ref=U_REF, smooth_uncert_max_gap=GAP)
        tester = POCOTester(a)
        Tn, H, W = 150, 96, 128
        r = np.random.default_rng(1)
        frames = [torch.from_numpy(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev) for _ in range(Tn)]
        tracking = {str(p): {"bbox": np.tile([[40.0 + 40 * p, 48.0, 60.0, 60.0]], (Tn, 1)).astype(np.float32), "frames": np.arange(Tn)}
                    for p in range(2)}
        tester.run_on_video(tracking, frames, W, H)
        rounds = {None: [], LAM: []}
        for _ in range(4):
            for flag in (None, LAM):
                a.smooth_uncert = flag
                rounds[flag].append(wall_ms(lambda: tester.run_on_video(tracking, frames, W, H), 3)[0])
        p_, f_ = statistics.median(rounds[None]), statistics.median(rounds[LAM])
        lines.append(f"(d) run_on_video 2 x {Tn} frames: plain {p_:.1f}  --smooth_uncert {LAM:g}: {f_:.1f}  difference: {f_ - p_:+.1f} "
                     f"= {100 * (f_ - p_) / p_:.1f} % of the plain run  "
                     f"(rounds plain {['%.1f' % v for v in rounds[None]]}, smoothed {['%.1f' % v for v in rounds[LAM]]})")
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
