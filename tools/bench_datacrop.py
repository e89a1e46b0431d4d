"""Input side of eval.py, two ways, timed on the GPU:

  batch   EvalDataset(crop='dataset'): each distinct image uploaded once, one poco_dataset_crop launch for the whole batch
  loop    what EvalDataset.batch(crop='demo') does per sample: upload the whole frame, one poco_crop_normalize launch for one box

at 1 / 16 / 64 / 128 crops cut from 1080p images, for one and for two people per image, as interleaved rounds in one process (the
decoded images are held in memory: PIL's decoding is the same on both sides and is not timed), and for ResNet-50-CLIFF at 64 crops
the forward behind each input side.  Times are host clocks around work that ends in a device synchronise, uploads included.

    python tools/bench_datacrop.py --out profiles/datacrop_step.txt [--rounds 7] [--reps 5]

A machine without a GPU is an error: nothing is estimated."""
import argparse
import json
import os
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
        sys.exit("bench_datacrop needs a GPU: nothing is estimated")
    from poco_amd import datacrop
    from poco_amd.tester import crop_normalize
    import bench
    dev = torch.device("cuda:0")
    r = np.random.default_rng(0)
    pool = [r.integers(0, 256, (1080, 1920, 3), dtype=np.uint8) for _ in range(8)]      # distinct 1080p frames, reused round-robin

    def sample(n, people):
        idx = [(i // people) for i in range(n)]
        center = np.column_stack([r.uniform(300, 1600, n), r.uniform(300, 800, n)]).astype(np.float32)
        scale = r.uniform(1.0, 3.0, n).astype(np.float32)
        return idx, center, scale

    def batch_side(idx, center, scale):
        n_img = idx[-1] + 1
        images = [datacrop.upload_image(pool[k % len(pool)], dev) for k in range(n_img)]
        n = len(idx)
        params = datacrop.batch_params(center, scale, np.zeros(n), np.zeros(n, np.int32), np.ones((n, 3)), np.ones(n), 224)
        return datacrop.dataset_crop(images, idx, params, 224, True)

    def loop_side(idx, center, scale):
        crops = []
        for i, k in enumerate(idx):
            side = float(scale[i]) * 200.0
            box = torch.tensor([[center[i, 0], center[i, 1], side, side]], dtype=torch.float32, device=dev)
            crops.append(crop_normalize(torch.from_numpy(pool[k % len(pool)]).to(dev), box, 1.0))
        return torch.cat(crops)

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    def compare(f_batch, f_loop):
        f_batch(), f_loop()                                # warm both shapes
        tb, tl = [], []
        for _ in range(a.rounds):                          # interleaved: batch, loop, batch, loop ...
            tb.append(timed(f_batch, a.reps))
            tl.append(timed(f_loop, a.reps))
        tb, tl = np.asarray(tb), np.asarray(tl)
        ratio = tl / tb
        return dict(batch_ms_median=float(np.median(tb)), batch_ms_min=float(tb.min()), batch_ms_max=float(tb.max()),
                    loop_ms_median=float(np.median(tl)), loop_ms_min=float(tl.min()), loop_ms_max=float(tl.max()),
                    ratio_median=float(np.median(ratio)), ratio_min=float(ratio.min()), ratio_max=float(ratio.max()))

    lines = [f"# tools/bench_datacrop.py on {torch.cuda.get_device_name(0)}: {a.rounds} interleaved rounds of {a.reps} batches; ms per batch, "
             "uploads included; ratio = loop / batch per round"]
    for people in (1, 2):
        for n in (1, 16, 64, 128):
            idx, center, scale = sample(n, people)
            row = dict(what="input_side", crops=n, people_per_image=people, images=idx[-1] + 1,
                       **compare(lambda: batch_side(idx, center, scale), lambda: loop_side(idx, center, scale)))
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    model = bench.build_model("resnet50-cliff", 64, dev)
    extra = {k: torch.from_numpy(v).to(dev) for k, v in __import__("poco_amd.synth", fromlist=["synth_batch"]).synth_batch(64, 77).items() if k != "img"}
    for people in (1, 2):
        idx, center, scale = sample(64, people)
        row = dict(what="forward_plus_input_side", variant="resnet50-cliff", crops=64, people_per_image=people,
                   **compare(lambda: model(dict(extra, img=batch_side(idx, center, scale)), want_segm=False),
                             lambda: model(dict(extra, img=loop_side(idx, center, scale)), want_segm=False)))
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    model.check_status()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
