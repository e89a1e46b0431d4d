"""Time the calibration operators (csrc/isotonic.hip), after warm-up:

    python tools/bench_calib.py [--iters 10] [--out profiles/calib_step.txt]

  (a) ops.isotonic (the launches + the wrapper's checks, the read-back of the offsets and its allocations) on ONE segment of
      1 000 / 35 515 / 852 360 rows: evaluation-like data (an error that rises with the key under heavy noise) and the adversarial
      patterns of tests/calib_np.py; device events around the Python call; the patterns of one size are timed in interleaved
      rounds, the median of the rounds' medians;
      beside it the host form on the same data (scipy.optimize.isotonic_regression on the unit means, wall clock);
  (b) the 28-segment call of a 35 515-crop evaluation: 3 segments over one sort of 35 515 rows, 1 of 852 360, 24 of 35 515;
  (c) ops.calib_apply at 64 x 27 and 35 515 x 27 on 27 maps;
  (d) eval.py's loop tail on an evaluator of 35 515 crops: finish() alone against finish() followed by calibrate.calibrate (26 sorts
      and one 28-segment fit; with a split three such fits and 56 scored maps); wall clock, synchronised.
Prints one line per measurement; --out also writes them to a file.  No pass / fail ratio."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from poco_amd import ops  # noqa: E402
from tests import calib_np  # noqa: E402
from tools.bench_rank import ROUNDS, rounds, wall_ms  # noqa: E402

CROPS = 35515
ADVERSARIAL = ("increasing", "decreasing", "one_unit", "saw_T", "huge_front", "huge_back", "halves", "small_ints")


def host_ms(fn, iters):
    """Wall clock of a pure host call: median, lowest, highest of `iters` after one warm-up."""
    fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(1000.0 * (time.perf_counter() - t0))
    return statistics.median(ts), min(ts), max(ts)


def host_form():
    try:
        from scipy.optimize import isotonic_regression
        return "scipy.optimize.isotonic_regression on the unit means", isotonic_regression
    except ImportError:
        return "tests/calib_np.py", None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    iters = max(args.iters, 3)
    dev = torch.device("cuda:0")
    label, iso_host = host_form()
    lines = [f"# tools/bench_calib.py on {torch.cuda.get_device_name(0)}: ms, median of {ROUNDS} interleaved rounds' medians of {iters} "
             f"calls (lowest .. highest round); device events around the Python call; host form ({label}): wall clock"]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)       # noqa: E731
    for n in (1000, CROPS, CROPS * 24):
        calls, hosts, heads = [], [], []
        for name in ("eval_like",) + ADVERSARIAL:                          # the patterns of one size are the interleaved legs
            key, y = calib_np.pattern(name, n, ops.ISO_TILE)
            dk, dy, do, ds = t(key, np.float32), t(y, np.float32), t(np.arange(n), np.int32), t([0, n], np.int32)
            scratch = torch.empty(ops.isotonic_scratch_bytes(n, 1), device=dev, dtype=torch.uint8)
            out = ops.isotonic(dk, dy, do, ds, scratch=scratch)
            heads.append(f"(a) isotonic n = {n:6d} {name:10s} ({int(out['seg_blocks'][1]):6d} blocks)")
            calls.append(lambda a=(dk, dy, do, ds), o=out, sc=scratch: ops.isotonic(*a, out=o, scratch=sc))

            def host(key=key, y=y, n=n):
                hd = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
                w = np.diff(np.concatenate([hd, [n]])).astype(np.float64)
                iso_host(np.add.reduceat(y.astype(np.float64), hd) / w, weights=w)
            hosts.append(host)
        for head, (a, alo, ahi), host in zip(heads, rounds(calls, iters), hosts):
            line = f"{head}: {a:.4f} ({alo:.4f} .. {ahi:.4f})"
            if iso_host is not None:
                h, hlo, hhi = host_ms(host, 7)
                line += f"   host: {h:.3f} ({hlo:.3f} .. {hhi:.3f})"
            lines.append(line)
            print(line, flush=True)
    # (b) 28 segments: rows 0..CROPS-1 three times (the crop maps), CROPS * 24 rows once, 24 planes of CROPS rows
    r = np.random.default_rng(1)
    M = CROPS + 2 * CROPS * 24
    key = r.gamma(2.0, 0.1, M).astype(np.float32)
    y = ((50.0 + 200.0 * key) * r.gamma(2.0, 0.5, M) + 1.0).astype(np.float32)
    parts, seg = [], [0]
    crop = np.argsort(key[:CROPS], kind="stable")
    for _ in range(3):
        parts.append(crop)
    parts.append(CROPS + np.argsort(key[CROPS:CROPS + CROPS * 24], kind="stable"))
    for j in range(24):
        lo = CROPS + CROPS * 24 + j * CROPS
        parts.append(lo + np.argsort(key[lo:lo + CROPS], kind="stable"))
    for p in parts:
        seg.append(seg[-1] + len(p))
    order = np.concatenate(parts)
    dk, dy, do, ds = t(key, np.float32), t(y, np.float32), t(order, np.int32), t(seg, np.int32)
    scratch = torch.empty(ops.isotonic_scratch_bytes(len(order), 28), device=dev, dtype=torch.uint8)
    out = ops.isotonic(dk, dy, do, ds, scratch=scratch)
    (a, alo, ahi), = rounds([lambda: ops.isotonic(dk, dy, do, ds, out=out, scratch=scratch)], iters)
    lines.append(f"(b) isotonic, 28 segments of a {CROPS}-crop evaluation, N = {len(order)} ({int(out['seg_blocks'][28])} blocks): "
                 f"{a:.4f} ({alo:.4f} .. {ahi:.4f})")
    # (c) the maps applied: 27 columns, column c uses map c + 1 of the 28 just fitted
    ids, offs = t(np.arange(1, 28), np.int32), out["seg_blocks"]
    knots = out["knots"][:int(offs[28])].contiguous()
    for R in (64, CROPS):
        x = torch.rand(R, 27, device=dev) * 1.5
        res = torch.empty_like(x)
        (a, alo, ahi), = rounds([lambda: ops.calib_apply(x, ids, offs, knots, out=res)], iters)
        lines.append(f"(c) calib_apply {R:6d} x 27: {a:.4f} ({alo:.4f} .. {ahi:.4f})")
    # (d) eval.py's loop tail on an evaluator of 35 515 crops: finish() alone against finish() followed by calibrate()
    from poco_amd import calibrate
    from tools.bench_rank import big_evaluator
    ev = big_evaluator(dev, CROPS)

    def tail():
        ev.finish()
        calibrate.calibrate(ev, "half", 20)

    def tail_none():
        ev.finish()
        calibrate.calibrate(ev, "none", 20)
    (a, alo, ahi), (b, blo, bhi), (c, clo, chi) = rounds([lambda: ev.finish(), tail_none, tail], 3, wall_ms)
    lines.append(f"(d) eval.py's loop tail, {CROPS} crops: finish(): {a:.2f} ({alo:.2f} .. {ahi:.2f})   finish() + calibrate(split none): "
                 f"{b:.2f} ({blo:.2f} .. {bhi:.2f})   finish() + calibrate(split half, 20 bins): {c:.2f} ({clo:.2f} .. {chi:.2f})")
    ev.close()
    print("\n".join(lines[-4:]))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
