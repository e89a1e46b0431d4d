"""The synthetic occluders of the dataset crop, timed on the GPU:

  batch   one poco_dataset_crop_occ launch for the whole batch, with 0 and with 7 objects per crop
  plain   poco_dataset_crop on the same crops (what the 0-object case is compared with)
  host    the path the device step replaces: poco_dataset_crop with normalize = 0 and no noise, download the raw crops, the numpy
          restatement's resize and paste per sample (tests/occlude_np.py, as the reference does it in numpy and cv2), upload, and
          noise / clamp / Normalize on the device in torch

at 1 / 16 / 64 / 128 crops cut from 1080p images that already lie on the device (the image uploads are the same on every side and
are section 22's subject), as interleaved rounds in one process.  Times are host clocks around work that ends in a device
synchronise; the records' upload is included.

    python tools/bench_occlude.py --out profiles/occlude_step.txt [--rounds 7] [--reps 5]

A machine without a GPU is an error: nothing is estimated."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="batches per round and side")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_occlude needs a GPU: nothing is estimated")
    from poco_amd import datacrop
    from tests import occlude_np
    dev = torch.device("cuda:0")
    r = np.random.default_rng(0)
    pool = [torch.from_numpy(r.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).to(dev) for _ in range(8)]
    # cut-outs of the sizes the reference's file holds after its 0.5 downscale: tens to a few hundred pixels a side
    cuts = []
    for h, w in r.integers(40, 250, (32, 2)):
        c = r.integers(0, 256, (int(h), int(w), 4), dtype=np.uint8)
        c[..., 3] = r.choice(np.array([0, 192, 255], np.uint8), (int(h), int(w)), p=[0.3, 0.1, 0.6])
        cuts.append(c)
    atlas = datacrop.OccluderAtlas(cuts, dev)
    sizes = [c.shape[:2] for c in cuts]
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)

    def sample(n, objects_per_crop):
        idx = [i % len(pool) for i in range(n)]
        center = np.column_stack([r.uniform(300, 1600, n), r.uniform(300, 800, n)]).astype(np.float32)
        scale = r.uniform(1.0, 3.0, n).astype(np.float32)
        params = datacrop.batch_params(center, scale, np.zeros(n), np.zeros(n, np.int32), np.ones((n, 3)), np.ones(n), 224)
        kp = np.concatenate([r.uniform(-0.7, 0.7, (24, 2)), np.ones((24, 1))], 1).astype(np.float32)
        np_rng, py_rng, objs = np.random.RandomState(1), random.Random(1), []
        for _ in range(n):
            o = []
            while len(o) < objects_per_crop:                     # the reference's draws, repeated until the crop has its objects
                o += datacrop.occlusion_params(np_rng, py_rng, kp, 1.0, sizes, 224)["objects"]
            objs.append(o[:objects_per_crop])
        return idx, params, objs, datacrop.occ_records(objs)

    def occ_side(idx, params, recs):
        return datacrop.dataset_crop(pool, idx, params, 224, True, occlusion=(atlas, recs))[0]

    def plain_side(idx, params):
        return datacrop.dataset_crop(pool, idx, params, 224, True)

    def host_side(idx, params, objs):
        raw = datacrop.dataset_crop(pool, idx, params, 224, False).permute(0, 2, 3, 1).cpu().numpy()
        done = np.stack([occlude_np.apply_objects_np(raw[n], cuts, objs[n])[0] for n in range(len(idx))])
        x = torch.from_numpy(done).to(dev).permute(0, 3, 1, 2)
        return (x.clamp(0, 255) / 255.0 - mean) / std

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    def compare(sides):
        for f in sides.values():
            f()                                                # warm every shape
        t = {k: [] for k in sides}
        for _ in range(a.rounds):                              # interleaved: one timing of every side per round
            for k, f in sides.items():
                t[k].append(timed(f, a.reps))
        t = {k: np.asarray(v) for k, v in t.items()}
        row = {}
        for k, v in t.items():
            row.update({f"{k}_ms_median": float(np.median(v)), f"{k}_ms_min": float(v.min()), f"{k}_ms_max": float(v.max())})
        first = next(iter(sides))
        for k in list(sides)[1:]:
            q = t[k] / t[first]
            row.update({f"{k}_over_{first}_median": float(np.median(q)), f"{k}_over_{first}_min": float(q.min()),
                        f"{k}_over_{first}_max": float(q.max())})
        return row

    lines = [f"# tools/bench_occlude.py on {torch.cuda.get_device_name(0)}: {a.rounds} interleaved rounds of {a.reps} batches; ms per batch of "
             "224 x 224 crops from resident 1080p images; ratios per round"]
    for n in (1, 16, 64, 128):
        idx, params, _, recs0 = sample(n, 0)
        row = dict(what="objects_0", crops=n, **compare({"occ": lambda: occ_side(idx, params, recs0), "plain": lambda: plain_side(idx, params)}))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        idx, params, objs, recs7 = sample(n, 7)
        row = dict(what="objects_7", crops=n, **compare({"occ": lambda: occ_side(idx, params, recs7), "host": lambda: host_side(idx, params, objs),
                                                         "plain": lambda: plain_side(idx, params)}))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
