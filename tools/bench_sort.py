"""Time SORT on the device (poco_amd/sort.py, csrc/sort_tracks.hip), after warm-up:

    python tools/bench_sort.py [--iters 30] [--out profiles/sort_step.txt]

  (a) ops.sort_tracks (one launch + the wrapper's checks, which download the boxes once), device events around the Python call, at
      1 / 8 clips x 300 / 3000 frames x 4 / 16 random walkers;
  (b) the numpy restatement tests/sort_np.py on the same input, wall clock, once (it is the contract written for reading, not a fast
      host tracker; inputs of more than 50 000 detections are not timed);
  (c) demo.py --mode video on 120 synthetic frames with 4 people, resnet50-cliff: --tracking FILE against --detections FILE
      --tracker sort, interleaved rounds, wall clock of the whole command.
Prints one line per measurement; --out also writes them to a file.  No pass / fail ratio."""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import ops, sort, synth  # noqa: E402
from tests import sort_np, util  # noqa: E402
from tools.bench_eval import event_ms  # noqa: E402
from tools.bench_infill import wall_ms  # noqa: E402


def walkers(r, C, T, P):
    """C clips of T frames with P people each: random walks 160 px apart, every person detected in every frame."""
    dets = np.empty((C, T, P, 4))
    for c in range(C):
        for i in range(P):
            steps = np.cumsum(r.normal(0, 2.0, (T, 2)), 0)
            size = 60 + np.cumsum(r.normal(0, 0.2, T))
            dets[c, :, i] = np.stack([150 + 160 * i + steps[:, 0], 300 + steps[:, 1], size, 2.2 * size], 1)
    fo = np.arange(C * T + 1, dtype=np.int32) * P
    co = np.arange(C + 1, dtype=np.int32) * T
    return dets.reshape(-1, 4), fo, co


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    iters = max(args.iters, 30)
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_sort.py on {torch.cuda.get_device_name(0)}, median (min .. max), ms"]
    for C in (1, 8):
        for T in (300, 3000):
            for P in (4, 16):
                dets, fo, co = walkers(np.random.default_rng(1000 * C + T + P), C, T, P)
                d = torch.from_numpy(dets).to(dev)
                res = ops.sort_tracks(d, fo, co)
                assert int(res["status"].max()) == 0
                med, lo, hi = event_ms(lambda: ops.sort_tracks(d, fo, co), iters)
                line = (f"(a) operator {C} clip(s) x {T} frames x {P} people: {med:.3f} ({lo:.3f} .. {hi:.3f}) = {1e3 * med / T:.2f} us per "
                        f"frame of a clip; trackers created per clip {res['count'].cpu().tolist()}")
                if len(dets) <= 50000:
                    t0 = time.perf_counter()
                    want = sort_np.sort_tracks(dets, fo, co)
                    host = 1e3 * (time.perf_counter() - t0)
                    same = all(np.array_equal(res[k].cpu().numpy(), want[k]) for k in ("tracker", "id", "count", "status"))
                    line += f"\n(b) numpy restatement, same input, once: {host:.0f}  restatement / operator = {host / med:.0f}  (same ids: {same})"
                else:
                    line += "\n(b) numpy restatement: not timed at this size"
                lines.append(line)
    # (c) video mode end to end: a tracking file against the tracks built from a detections file
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
        names = [f"{i:06d}.png" for i in range(T)]
        dets = {n: [[16.0 + 32 * p + 0.05 * i, 48.0 + 0.02 * i * (p - 1.5), 24.0, 60.0] for p in range(P)] for i, n in enumerate(names)}
        (tmp / "dets.json").write_text(json.dumps(dets))
        tracks = sort.build_tracks(dets, names)
        assert len(tracks) == P
        sort.write_tracking(str(tmp / "tracks.json"), tracks)
        common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "poco_synth.pt"), "--mode", "video", "--vid_file",
                  str(tmp / "frames"), "--batch_size", "64", "--smpl", str(tmp / "smpl.npz"), "--no_render", "--output_folder", str(tmp / "out")]
        forms = {"tracking": ["--tracking", str(tmp / "tracks.json")], "sort": ["--detections", str(tmp / "dets.json"), "--tracker", "sort"]}
        rounds = {k: [] for k in forms}
        for k, flags in forms.items():                                   # warm-up: one run of each
            demo.main(demo.parse_args(common + flags))
        for _ in range(5):
            for k, flags in forms.items():
                rounds[k].append(wall_ms(lambda: demo.main(demo.parse_args(common + flags)), 1)[0])
        a, b = statistics.median(rounds["tracking"]), statistics.median(rounds["sort"])
        lines.append(f"(c) demo.py --mode video, {T} frames x {P} people, engine build included: --tracking {a:.0f}  --tracker sort {b:.0f}  "
                     f"difference {b - a:+.0f} = {100 * (b - a) / a:+.1f} %  (rounds tracking {['%.0f' % v for v in rounds['tracking']]}, "
                     f"sort {['%.0f' % v for v in rounds['sort']]})")
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
