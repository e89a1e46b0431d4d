"""Time the cluster bootstrap (csrc/bootstrap.hip, poco_amd/bootstrap.py), after warm-up:

    python tools/bench_boot.py [--iters 5] [--out profiles/boot_step.txt]

  (a) ops.bootstrap (its launches + the wrapper's checks; outputs and scratch allocated once) at U = 1 000 and 35 515 crop units (every
      row a unit) and at 60 track units over 35 515 rows, each with B = 200 and 2 000 and with M = 13 (E = 6, P = 6) and M = 10 (E = 4,
      P = 5); device events around the Python call; the shapes are timed in interleaved rounds, the median of the rounds' medians;
  (b) beside each, the vectorised numpy form on the same draws on 16 threads: unit_mom[idx[b]].sum(0) per replicate from the device's
      unit moments (wall clock; the draws - tests/boot_np.draws_np - are timed apart);
  (c) eval.py's loop tail on an evaluator of 35 515 crops: finish() alone against finish() followed by bootstrap_evaluators with
      B = 2 000 (two operator calls, two read-backs of [B + 1, M] and the statistics); wall clock, synchronised.
Prints one line per measurement; --out also writes them to a file.  No pass / fail ratio."""
import argparse
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import bootstrap, ops  # noqa: E402
from tests import boot_np  # noqa: E402
from tools.bench_rank import ROUNDS, big_evaluator, rounds, wall_ms  # noqa: E402

CROPS = 35515
THREADS = 16
SHAPES = (("crop", 1000, None), ("crop", CROPS, None), ("track", CROPS, 60))
COLUMNS = ((6, 6), (4, 5))


def host_ms(fn, iters):
    fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(1000.0 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    iters = max(args.iters, 3)
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_boot.py on {torch.cuda.get_device_name(0)}: ms, median of {ROUNDS} interleaved rounds' medians of {iters} calls "
             f"(lowest .. highest round); device events around the Python call; numpy form on {THREADS} threads: wall clock, median of 3"]
    r = np.random.default_rng(0)
    calls, heads, hosts = [], [], []
    pool = ThreadPoolExecutor(THREADS)
    for unit, n, tracks in SHAPES:
        offsets = None
        if tracks:
            cuts = np.sort(r.choice(np.arange(1, n), tracks - 1, replace=False))
            offsets = torch.from_numpy(np.concatenate([[0], cuts, [n]]).astype(np.int32)).to(dev)
        U = tracks or n
        for E, P in COLUMNS:
            planes = torch.from_numpy(r.gamma(2.0, 0.05, (E, n)).astype(np.float32)).to(dev)
            pairs = [(k % E, (2 * k + 1) % E) for k in range(P)]
            scratch = torch.empty(ops.bootstrap_scratch_bytes(n, E, P, U), device=dev, dtype=torch.uint8)
            for B in (200, 2000):
                out = ops.bootstrap(planes, pairs, offsets, B, 1, scratch=scratch)
                heads.append(f"(a) bootstrap {unit:5s} units U = {U:5d} of n = {n:5d} rows, M = {1 + E + P:2d}, B = {B:4d}")
                calls.append(lambda a=(planes, pairs, offsets, B, 1), o=out, sc=scratch: ops.bootstrap(*a, out=o, scratch=sc))
                mom = out["unit_mom"].cpu().numpy()

                def draw(B=B, U=U):
                    return list(pool.map(lambda b: boot_np.draws_np(1, b, U), range(1, B + 1)))
                hosts.append((draw, mom))
    for head, (a, alo, ahi), (draw, mom) in zip(heads, rounds(calls, iters), hosts):
        idx = draw()
        d, s = host_ms(draw, 3), host_ms(lambda: list(pool.map(lambda i: mom[i].sum(axis=0), idx)), 3)
        del idx
        line = f"{head}: {a:.4f} ({alo:.4f} .. {ahi:.4f})   numpy: draws {d[0]:.1f} ({d[1]:.1f} .. {d[2]:.1f}) + sums {s[0]:.1f} ({s[1]:.1f} .. {s[2]:.1f})"
        lines.append(line)
        print(line, flush=True)
    pool.shutdown()
    # (c) eval.py's loop tail on an evaluator of 35 515 crops
    ev = big_evaluator(dev, CROPS)
    spec = bootstrap.BootSpec(2000)

    def tail():
        ev.finish()
        bootstrap.bootstrap_evaluators([("", ev)], spec)
    (a, alo, ahi), (b, blo, bhi) = rounds([lambda: ev.finish(), tail], 3, wall_ms)
    lines.append(f"(c) eval.py's loop tail, {CROPS} crops: finish(): {a:.2f} ({alo:.2f} .. {ahi:.2f})   finish() + bootstrap_evaluators(B = 2000, "
                 f"crop units): {b:.2f} ({blo:.2f} .. {bhi:.2f})")
    ev.close()
    print(lines[-1])
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
