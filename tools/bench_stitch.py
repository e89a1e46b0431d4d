"""Time the track stitcher on the device (poco_amd/stitch.py, csrc/track_stitch.hip), after warm-up:

    python tools/bench_stitch.py [--iters 30] [--out profiles/stitch_step.txt]

  (a) ops.track_stitch (three launches + the wrapper's checks, which download the rows once), device events around the Python call,
      at 1 / 8 clips x 16 / 256 fragments x 30 / 300 rows: walkers seen for a while, hidden for 5 frames, seen again;
  (b) the numpy restatement tests/stitch_np.py on the same input, wall clock, once (it is the contract written for reading; inputs of
      more than 64 fragments a clip or 20 000 rows are not timed);
  (c) demo.py --mode video on 120 synthetic frames with 4 people who each miss 5 frames, resnet50-cliff, --tracker sort: without and
      with --track_stitch, interleaved rounds, wall clock of the whole command.
Prints one line per measurement; --out also writes them to a file.  No pass / fail ratio."""
import argparse
import pickle
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import ops, synth  # noqa: E402
from tests import stitch_np, util  # noqa: E402
from tools.bench_eval import event_ms  # noqa: E402
from tools.bench_infill import wall_ms  # noqa: E402


def fragments(r, C, P, T):
    """C clips of P fragments of T rows: P / 2 walkers 200 px apart, each seen for T frames, hidden for 5, seen for T again."""
    co, fo, fr, bx, be, va = [0], [0], [], [], [], []
    for _ in range(C):
        for half in (0, 1):
            for i in range(P // 2):
                f = np.arange(T) + half * (T + 5)
                shape = np.random.default_rng(i).normal(0, 1, 10)
                fr.append(f)
                bx.append(np.stack([100 + 200.0 * i + 1.5 * f, 300 + 0.5 * f, 40 + 0 * f, 90 + 0.05 * f], 1) + r.normal(0, 0.2, (T, 4)))
                be.append(shape[None] + r.normal(0, 0.02, (T, 10)))
                va.append(0.1 + 0.05 * r.random((T, 24)))
                fo.append(fo[-1] + T)
        co.append(co[-1] + P)
    return (np.asarray(co, np.int32), np.asarray(fo, np.int32), np.concatenate(fr).astype(np.int32), np.concatenate(bx),
            np.concatenate(be).astype(np.float32), np.concatenate(va).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    iters = max(args.iters, 30)
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_stitch.py on {torch.cuda.get_device_name(0)}, median (min .. max), ms"]
    for C in (1, 8):
        for P in (16, 256):
            for T in (30, 300):
                co, fo, *rows = fragments(np.random.default_rng(1000 * C + P + T), C, P, T)
                d = [torch.from_numpy(a).to(dev) for a in rows]
                res = ops.track_stitch(co, fo, *d)
                assert int(res["status"].max()) == 0
                links = int((res["succ"] >= 0).sum())
                med, lo, hi = event_ms(lambda: ops.track_stitch(co, fo, *d), iters)
                line = f"(a) operator {C} clip(s) x {P} fragments x {T} rows: {med:.3f} ({lo:.3f} .. {hi:.3f}); links {links} of {C * P // 2}"
                if P <= 64 and len(rows[0]) <= 20000:
                    t0 = time.perf_counter()
                    want = stitch_np.track_stitch(co, fo, *rows)
                    host = 1e3 * (time.perf_counter() - t0)
                    same = all(np.array_equal(res[k].cpu().numpy(), want[k]) for k in ("succ", "pred", "chain", "status"))
                    line += f"\n(b) numpy restatement, same input, once: {host:.0f}  restatement / operator = {host / med:.0f}  (same links: {same})"
                else:
                    line += "\n(b) numpy restatement: not timed at this size"
                lines.append(line)
    # (c) video mode end to end: SORT's tracks as they are against the same tracks stitched
    with tempfile.TemporaryDirectory() as tmp:
        from PIL import Image
        import demo
        tmp = Path(tmp)
        T, H, W, P = 120, 96, 128, 4
        w = util.synth_weights("resnet50-cliff")
        torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "poco_synth.pt")
        np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
        (tmp / "frames").mkdir()
        r = np.random.default_rng(5)
        for i in range(T):
            Image.fromarray(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(tmp / "frames" / f"{i:06d}.png")
        dets = {f"{i:06d}.png": np.asarray([[16.0 + 32 * p + 0.05 * i, 48.0 + 0.02 * i * (p - 1.5), 24.0, 60.0] for p in range(P)
                                            if not 40 + 10 * p <= i < 45 + 10 * p], np.float32).reshape(-1, 4) for i in range(T)}
        with open(tmp / "dets.pkl", "wb") as f:
            pickle.dump(dets, f)
        common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "poco_synth.pt"), "--mode", "video", "--vid_file",
                  str(tmp / "frames"), "--batch_size", "64", "--smpl", str(tmp / "smpl.npz"), "--no_render", "--output_folder", str(tmp / "out"),
                  "--detections", str(tmp / "dets.pkl"), "--tracker", "sort", "--track_backfill"]
        forms = {"plain": [], "stitch": ["--track_stitch", "--stitch_shape", "0"]}
        rounds = {k: [] for k in forms}
        for k, flags in forms.items():                                   # warm-up: one run of each
            demo.main(demo.parse_args(common + flags))
        for _ in range(5):
            for k, flags in forms.items():
                rounds[k].append(wall_ms(lambda: demo.main(demo.parse_args(common + flags)), 1)[0])
        a, b = statistics.median(rounds["plain"]), statistics.median(rounds["stitch"])
        lines.append(f"(c) demo.py --mode video --tracker sort, {T} frames x {P} people with one 5-frame hole each, engine build included: "
                     f"plain {a:.0f}  --track_stitch {b:.0f}  difference {b - a:+.0f} = {100 * (b - a) / a:+.1f} %  "
                     f"(rounds plain {['%.0f' % v for v in rounds['plain']]}, stitch {['%.0f' % v for v in rounds['stitch']]})")
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
