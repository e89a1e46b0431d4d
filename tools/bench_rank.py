"""Time the rank-based uncertainty metrics (poco_amd/ranking.py, csrc/rank_curve.hip), after warm-up:

    python tools/bench_rank.py [--iters 20] [--out profiles/rank_step.txt]

  (a) the operator (16 launches + the wrapper's checks and allocations) at n = 1 000 / 35 515 / 852 360 rows (3DPW per crop and per
      joint) with E = 1 and E = 3 value planes, K = 20, against the torch form on the same GPU: torch.argsort(stable=True), a gather
      of every plane, cumsum in float64 (no midranks, which the operator also writes); and poco_op_pearson64 on two rank arrays
      against torch.corrcoef; device events around the Python call, interleaved rounds, the median of the rounds' medians;
  (b) the host form at 3DPW's size: Evaluator.finish(return_records=True), then per joint numpy's stable argsort of the
      uncertainty and scipy.stats.rankdata of both columns; wall clock around the call;
  (c) eval.py's loop tail on the same evaluator (35 515 crops on a 431-vertex mesh): finish() alone against finish() followed by
      ranking.RankMetrics(K = 20) (both modes: 6 sorts, 4 correlations, the read-back of the cut sums); wall clock, synchronised.
Prints one line per measurement; --out also writes them to a file.  No pass / fail ratio."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import scipy.stats
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import evaluate, ops, ranking  # noqa: E402
from tests import eval_np  # noqa: E402
from tools.bench_eval import event_ms  # noqa: E402

ROUNDS = 3
CROPS = 35515


def rounds(fns, iters, timer=event_ms):
    """Interleaved rounds of the given callables; per callable the median of its rounds' medians and the spread of those."""
    meds = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            meds[i].append(timer(fn, iters)[0])
    return [(statistics.median(m), min(m), max(m)) for m in meds]


def wall_ms(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1000.0 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def torch_form(key, vals, K):
    """Sort, gather, prefix sums with torch on the device: the baseline of (a).  Cut sums of the key and of every plane."""
    n = key.shape[0]
    order = torch.argsort(key, stable=True)
    planes = torch.cat([key[None], vals]).double()[:, order]
    cs = torch.cumsum(planes, 1)
    c = torch.tensor([(k * n) // K for k in range(1, K + 1)], device=key.device) - 1
    return order, cs[:, c]


def big_evaluator(dev, crops):
    """An Evaluator on a 431-vertex mesh stepped to `crops` records in batches of 2048 (distinct uncertainties and errors)."""
    r = np.random.default_rng(3)
    V = 431
    Jr = np.zeros((17, V), np.float32)
    for j in range(17):
        Jr[j, r.choice(V, 6, replace=False)] = r.dirichlet(np.ones(6)).astype(np.float32)
    ev = evaluate.Evaluator(Jr, evaluate.joint_map("3dpw"), capacity=crops, device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)   # noqa: E731
    for lo in range(0, crops, 2048):
        B = min(2048, crops - lo)
        gt = r.uniform(-0.5, 0.5, (B, V, 3))
        pred = gt + 0.02 * r.standard_normal(gt.shape) * r.uniform(0.2, 3, (B, 1, 1))
        pose = r.uniform(-1, 1, (B, 72))
        pp = eval_np.rodrigues(pose.reshape(-1, 3) + 0.1 * r.standard_normal((B * 24, 3)), np.float64).reshape(B, 24, 3, 3)
        ev.step({"smpl_vertices": t(pred), "pred_pose": t(pp), "var_pose": t(r.uniform(0, 1, (B, 24)))}, t(pose), gt_vertices=t(gt))
    return ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    iters = max(args.iters, 5)
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_rank.py on {torch.cuda.get_device_name(0)}: ms, median of {ROUNDS} interleaved rounds' medians of {iters} "
             "calls (lowest .. highest round); (a) device events around the Python call, (b) (c) wall clock"]
    g = torch.Generator(device=dev).manual_seed(0)
    K = 20
    for n in (1000, CROPS, CROPS * 24):
        key = torch.rand(n, device=dev, generator=g)
        for E in (1, 3):
            vals = torch.rand(E, n, device=dev, generator=g)
            op = lambda: ops.rank_curve(key, vals, K)                                         # noqa: E731
            ref = lambda: torch_form(key, vals, K)                                            # noqa: E731
            (a, alo, ahi), (b, blo, bhi) = rounds([op, ref], iters)
            lines.append(f"(a) operator n = {n:6d}, E = {E}, K = {K}: {a:.4f} ({alo:.4f} .. {ahi:.4f})   torch (argsort stable, gather, cumsum "
                         f"float64): {b:.4f} ({blo:.4f} .. {bhi:.4f})")
        ra, rb = ops.rank_curve(key, None, 1)["rank"], ops.rank_curve(vals[0].contiguous(), None, 1)["rank"]
        both = torch.stack([ra, rb])
        (a, alo, ahi), (b, blo, bhi) = rounds([lambda: ops.pearson64(ra, rb), lambda: torch.corrcoef(both)], iters)
        lines.append(f"(a) pearson64 n = {n:6d}: {a:.4f} ({alo:.4f} .. {ahi:.4f})   torch.corrcoef float64: {b:.4f} ({blo:.4f} .. {bhi:.4f})")
    ev = big_evaluator(dev, CROPS)

    def host_form():
        res = ev.finish(return_records=True)
        np.argsort(res["corr_y"], kind="stable")
        scipy.stats.rankdata(res["corr_y"])
        scipy.stats.rankdata(res["corr_x"])

    def tail_ranked():
        ev.finish()
        ranking.RankMetrics(ev, K)
    few = max(iters // 4, 3)
    (h, hlo, hhi), = rounds([host_form], few, wall_ms)
    lines.append(f"(b) host form, {CROPS} crops: finish(return_records), numpy stable argsort and scipy rankdata x 2 of {CROPS * 24} pairs: "
                 f"{h:.2f} ({hlo:.2f} .. {hhi:.2f})")
    (a, alo, ahi), (b, blo, bhi) = rounds([lambda: ev.finish(), tail_ranked], few, wall_ms)
    lines.append(f"(c) eval.py's loop tail, {CROPS} crops: finish(): {a:.2f} ({alo:.2f} .. {ahi:.2f})   finish() + RankMetrics(K = {K}): "
                 f"{b:.2f} ({blo:.2f} .. {bhi:.2f})")
    ev.close()
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
