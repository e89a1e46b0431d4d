"""Time test-time augmentation (poco_amd/tta.py, csrc/tta_fuse.hip), after warm-up:

    python tools/bench_tta.py [--iters 30] [--out profiles/tta_step.txt]

  (a) the operator (one launch + the wrapper's checks and allocations) at 1 / 16 / 64 / 128 crops x K = 2, 4, 8 views in both
      weights, against the same fusion written in torch on the device (index, torch.linalg.svd, det fix; float64, no dropped
      views); device events around the Python call, interleaved rounds, the median of the rounds' medians;
  (b) TTAModel's forward (the engine on K * b rows + the operator + LBS of the b fused rows) against the engine's forward of the
      same K * b rows alone, resnet50-cliff, K * b = 64, the same way - the forward alone is what the engine did before;
  (c) eval.py's loop over 128 samples cut with the dataset crop from eight 320 x 240 images, batch size 64: evaluate.run_eval
      (crop='dataset') against evaluate.run_eval_tta with --tta flip (twice the rows through the engine, three evaluators, three
      finish() calls); the call includes reading the images, the uploads and the read-back of the records.
Prints one line per measurement; --out also writes them to a file.  No pass / fail ratio."""
import argparse
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import evaluate, ops, synth, tta  # noqa: E402
from poco_amd.datacrop import SMPL_JOINTS_FLIP_PERM  # noqa: E402
from tests import util  # noqa: E402
from tools.bench_eval import event_ms  # noqa: E402

ROUNDS = 5
VIEWS8 = [(0, 0.0), (1, 0.0), (0, 15.0), (1, 15.0), (0, -15.0), (1, -15.0), (0, 30.0), (0, -30.0)]


def torch_fuse(pose, var, betas, views, weight):
    """The same fusion with torch on the device, in float64: the baseline of (a).  No view is dropped."""
    K = len(views)
    P, V, Bt = pose.view(K, -1, 24, 3, 3).double(), var.view(K, -1, 24).double(), betas.view(K, -1, 10).double()
    perm = torch.tensor(SMPL_JOINTS_FLIP_PERM, device=pose.device)
    m = torch.tensor([1.0, -1.0, -1.0], device=pose.device, dtype=torch.float64)
    D = m[:, None] * m[None, :]
    Rs, Vs = [], []
    for k, (flip, rot) in enumerate(views):
        R, v = P[k], V[k]
        if flip:
            R, v = R.index_select(1, perm) * D, v.index_select(1, perm)
        if rot:
            c, s = ops.tta_view_cs(rot)
            Rz = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], device=pose.device, dtype=torch.float64)
            R = torch.cat([Rz @ R[:, :1], R[:, 1:]], 1)
        Rs.append(R)
        Vs.append(v)
    R, v = torch.stack(Rs), torch.stack(Vs)
    w = 1.0 / (v + 1e-9) if weight == "uncert" else torch.ones_like(v)
    W = w.sum(0)
    M = (w[..., None, None] * R).sum(0)
    U, _, Vh = torch.linalg.svd(M)
    U = torch.cat([U[..., :2], U[..., 2:] * torch.det(U @ Vh)[..., None, None]], -1)
    Rp = U @ Vh
    spread = (w * ((R - Rp) ** 2).mean((-1, -2))).sum(0) / W
    g = w[:, :, 0]
    return Rp.float(), ((w * v).sum(0) / W).float(), spread.float(), ((g[..., None] * Bt).sum(0) / g.sum(0)[:, None]).float()


def rounds(fns, iters):
    """Interleaved rounds of the given callables; per callable the median of its rounds' medians and the spread of those."""
    meds = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            meds[i].append(event_ms(fn, iters)[0])
    return [(statistics.median(m), min(m), max(m)) for m in meds]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    iters = max(args.iters, 10)
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_tta.py on {torch.cuda.get_device_name(0)}: ms, median of {ROUNDS} interleaved rounds' medians of {iters} "
             "calls (lowest .. highest round), device events around the Python call"]
    r = np.random.default_rng(0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)   # noqa: E731
    for B in (1, 16, 64, 128):
        for K in (2, 4, 8):
            views = VIEWS8[:K]
            q = r.standard_normal((K * B * 24, 4))
            q /= np.linalg.norm(q, axis=1, keepdims=True)
            w_, x, y, z = q.T
            rot = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y), 2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z),
                            2 * (y * z - w_ * x), 2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)], 1)
            pose, var, betas = t(rot.reshape(K * B, 24, 3, 3)), t(r.uniform(0.01, 0.5, (K * B, 24))), t(r.standard_normal((K * B, 10)))
            for weight in tta.WEIGHTS:
                op = lambda: ops.tta_fuse(pose, var, betas, views, weight)                    # noqa: E731
                ref = lambda: torch_fuse(pose, var, betas, views, weight)                     # noqa: E731
                (a, alo, ahi), (b, blo, bhi) = rounds([op, ref], iters)
                lines.append(f"(a) operator {B:3d} crops x {K} views, {weight:7s}: {a:.4f} ({alo:.4f} .. {ahi:.4f})   torch (index, svd, det fix): "
                             f"{b:.4f} ({blo:.4f} .. {bhi:.4f})")
    R = 64
    m0 = util.make_engine("resnet50-cliff", max_batch=R, seed=0)
    batch = {"img": t(r.standard_normal((R, 3, 224, 224))), "bbox_info": t(r.standard_normal((R, 3)) * 0.1),
             "focal_length": t(np.full(R, 1500.0)), "scale": t(np.full(R, 1.2)), "center": t(np.tile([[640.0, 360.0]], (R, 1))),
             "orig_shape": t(np.tile([[720.0, 1280.0]], (R, 1)))}
    fns, names = [lambda: m0(batch, want_segm=False)], [f"the engine's forward of {R} rows alone"]
    for text in ("flip", "flip,rot:15,rot:-15", "flip,rot:15,rot:-15,flip+rot:15,flip+rot:-15,scale:1.1,scale:0.9"):
        model = tta.TTAModel(m0, tta.parse_views(text), "uncert")
        fns.append(lambda model=model: model(batch))
        names.append(f"forward + fuse + LBS, K = {model.K} ({R // model.K} crops)")
    for name, (a, lo, hi) in zip(names, rounds(fns, max(iters // 3, 5))):
        lines.append(f"(b) resnet50-cliff, {R} rows, {name}: {a:.3f} ({lo:.3f} .. {hi:.3f})")
    N = 128
    with tempfile.TemporaryDirectory() as tmp:
        from PIL import Image
        tmp = Path(tmp)
        (tmp / "imgs").mkdir()
        for i in range(8):
            Image.fromarray(r.integers(0, 256, (240, 320, 3), dtype=np.uint8)).save(tmp / "imgs" / f"{i}.png")
        np.savez(tmp / "ds.npz", imgname=np.array([f"{i % 8}.png" for i in range(N)]), center=r.uniform([120, 90], [200, 150], (N, 2)).astype(np.float32),
                 scale=r.uniform(0.5, 1.0, N).astype(np.float32), pose=(r.standard_normal((N, 72)) * 0.2).astype(np.float32),
                 shape=r.standard_normal((N, 10)).astype(np.float32))
        ds = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset")
        J = synth.synth_j_regressor_h36m(11)
        model = tta.TTAModel(m0, tta.parse_views("flip"), "uncert")
        fns = [lambda: evaluate.run_eval(m0, ds, J, batch_size=R), lambda: evaluate.run_eval_tta(model, ds, J, batch_size=R)]
        names = ["plain (run_eval, crop='dataset')", "--tta flip (run_eval_tta)"]
        for name, (a, lo, hi) in zip(names, rounds(fns, max(iters // 3, 5))):
            lines.append(f"(c) eval.py's loop, {N} samples, batch size {R}, {name}: {a:.3f} ({lo:.3f} .. {hi:.3f})")
    m0.check_status(sync=True)
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
