"""Time video mode's in-fill (poco_amd/infill.py, csrc/track_infill.hip), after warm-up:

    python tools/bench_infill.py [--iters 30] [--out profiles/infill_step.txt]

  (a) the operator alone (two launches), device events around the Python call, at 1 / 8 tracks x 300 / 3000 frames with 10 % of the
      entries unreliable, in runs;
  (b) the whole step on the same tracks, wall clock: infill_tracks = upload of the ragged buffer, the operator, LBS of the touched
      rows, download and scatter;
  (c) the host path it stands in for, wall clock: tests/infill_np.py (float64 loops) + LBS of every row of every track;
  (d) one synthetic clip (2 tracks x 150 frames of 96 x 128, resnet50-cliff, batch 64) through POCOTester.run_on_video with and
      without --infill, interleaved rounds.
Prints one line per measurement; --out also writes them to a file.  No pass / fail ratio."""
import argparse
import statistics
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import infill, ops, synth  # noqa: E402
from tests import infill_np, util  # noqa: E402
from tools.bench_eval import event_ms  # noqa: E402

THR, GAP = 0.5, 30


def make_tracks(P, T, seed):
    r = np.random.default_rng(seed)
    tracks = {}
    for p in range(P):
        bad = np.zeros((T, 24), bool)
        for j in range(24):
            while bad[:, j].mean() < 0.1:
                t = int(r.integers(0, T))
                bad[t:t + int(r.integers(1, 13)), j] = True
        R = infill_np.smooth_rotations(r, 64, 2.0)
        tracks[str(p)] = {"pose": np.tile(R, (T // 64 + 1, 1, 1, 1))[:T].copy(), "betas": r.standard_normal((T, 10)).astype(np.float32),
                          "orig_cam": r.standard_normal((T, 4)).astype(np.float32), "frame_ids": np.arange(T),
                          "var": np.where(bad, 0.9, 0.1).astype(np.float32), "verts": np.zeros((T, 6890, 3), np.float32),
                          "smpl_joints3d": np.zeros((T, 49, 3), np.float32)}
    return tracks


def wall_ms(fn, n):
    fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    iters = max(args.iters, 30)
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_infill.py on {torch.cuda.get_device_name(0)}, median (min .. max), ms; thresh {THR}, max_gap {GAP}, "
             "10 % of the entries unreliable in runs of 1 .. 12 rows"]
    model = util.make_engine("resnet50-cliff", max_batch=64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    for P, T in ((1, 300), (8, 300), (1, 3000), (8, 3000)):
        tracks = make_tracks(P, T, 100 * P + T)
        cat = lambda k: np.concatenate([tr[k] for tr in tracks.values()])                         # noqa: E731
        pose, var, frames = cat("pose"), cat("var"), cat("frame_ids").astype(np.int32)
        lin = np.concatenate([cat("betas"), cat("orig_cam")], 1)
        offsets = np.arange(P + 1, dtype=np.int32) * T
        dp, du, df, dl, do = t(pose), t(var), t(frames), t(lin), torch.from_numpy(offsets)
        med, lo, hi = event_ms(lambda: ops.track_infill(dp, du, df, do, dl, THR, GAP, rows=True), iters)
        lines.append(f"(a) operator {P} x {T}: {med:.4f} ({lo:.4f} .. {hi:.4f})  [two launches + the wrapper's checks and allocations]")
        res = infill.infill_tracks(model, tracks, THR, GAP)
        touched = sum(r["counts"]["touched_frames"] for r in res.values())
        med, lo, hi = wall_ms(lambda: infill.infill_tracks(model, tracks, THR, GAP), 10)
        lines.append(f"(b) step {P} x {T} ({touched} of {P * T} rows re-posed): {med:.2f} ({lo:.2f} .. {hi:.2f})")

        def host():
            out = infill_np.infill(pose, var, frames, offsets, lin, THR, GAP)
            for lo_ in range(0, P * T, 64):
                v, j = model.smpl_lbs(t(out["lin"][lo_:lo_ + 64, :10]), t(out["pose"][lo_:lo_ + 64]))
                v.cpu(), j.cpu()

        med, lo, hi = wall_ms(host, 3 if P * T <= 3000 else 1)
        lines.append(f"(c) host path {P} x {T} (infill_np float64 + LBS of all {P * T} rows): {med:.1f} ({lo:.1f} .. {hi:.1f})")
    del model
    # (d) video mode with and without the flag
    from poco_amd.tester import POCOTester
    with tempfile.TemporaryDirectory() as tmp:
        w = util.synth_weights("resnet50-cliff")
        torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, f"{tmp}/w.pt")
        np.savez(f"{tmp}/smpl.npz", **synth.synth_smpl(7))
        a = SimpleNamespace(cfg=str(ROOT / "configs" / "demo_poco_cliff_resnet50.yaml"), ckpt=f"{tmp}/w.pt", batch_size=64, smpl=f"{tmp}/smpl.npz",
                            infill=None, infill_max_gap=GAP, smooth=False)
        tester = POCOTester(a)
        Tn, H, W = 150, 96, 128
        r = np.random.default_rng(1)
        frames = [torch.from_numpy(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev) for _ in range(Tn)]
        tracking = {str(p): {"bbox": np.tile([[40.0 + 40 * p, 48.0, 60.0, 60.0]], (Tn, 1)).astype(np.float32), "frames": np.arange(Tn)}
                    for p in range(2)}
        plain = tester.run_on_video(tracking, frames, W, H)
        thr = float(np.median(np.concatenate([v["var"][:, 0] for v in plain.values()])))
        rounds = {None: [], thr: []}
        for _ in range(4):
            for flag in (None, thr):
                a.infill = flag
                rounds[flag].append(wall_ms(lambda: tester.run_on_video(tracking, frames, W, H), 3)[0])
        p_, f_ = statistics.median(rounds[None]), statistics.median(rounds[thr])
        lines.append(f"(d) run_on_video 2 x {Tn} frames: plain {p_:.1f}  --infill {thr:.4g}: {f_:.1f}  difference: {f_ - p_:+.1f}  "
                     f"(rounds plain {['%.1f' % v for v in rounds[None]]}, infill {['%.1f' % v for v in rounds[thr]]})")
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
