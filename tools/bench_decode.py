"""Time the JPEG decoder (poco_jpeg_decode: one copy, the synchronisation rounds, counts, write, DC scan, inverse DCT, colour) with
HIP events at 1920 x 1080 for 1, 16 and 64 images per call, on a photo-like and on a noise picture (4:2:0, quality 90, written by
PIL), once without restart markers and once with one interval per MCU row - and, in the same run, the path it replaces: PIL decode
on a thread pool of the tester's size plus the pinned upload.  One JSON line per case, also appended to profiles/decode.txt.

    python tools/bench_decode.py [--iters 50] [--folder 16]
Every case runs in a child process of its own under a time limit, so a case that hangs ends alone.
--folder N: also the folder-mode wall time per image of demo.py on N synthetic 1080p .jpg images with --decode host and --decode gpu.

    python tools/bench_decode.py --png [--folder 16]
The PNG decoder (poco_png_decode: one copy, inflate, unfilter) instead, 5 repeats per case, against PIL decode on 16 threads plus
the upload; the files are a photo-like frame saved by PIL at its default level and the same frame from this project's PngEncoder.
Writes profiles/decode_png.txt; --folder N times folder mode with and without --decode_png gpu.

    python tools/bench_decode.py --progressive [--folder 16]
The progressive JPEG decoder (poco_jpeg_prog_decode: one copy, one launch per level of the scan order, inverse DCT, colour) on the
photo-like frame saved by PIL as a progressive 4:2:0 file of quality 90 (10 scans), measured as the PNG decoder is.  Writes
profiles/decode_progressive.txt; --folder N times folder mode per setting of --decode_progressive."""
import argparse
import io
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
H, W = 1080, 1920
POOL = 8                                   # the tester's pool size on a machine with 16 or more CPUs


def picture(kind):
    r = np.random.default_rng(0)
    if kind == "noise":
        return r.integers(0, 256, (H, W, 3), dtype=np.uint8)
    g = np.linspace(0, 255, W)[None, :, None] * np.array([1.0, 0.6, 0.3])
    img = g + np.linspace(0, 60, H)[:, None, None]
    y, x = np.mgrid[0:H, 0:W]
    img[(x // 120 + y // 90) % 5 == 0] *= 0.4                                   # hard edges
    img += r.normal(0, 4, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def stream(kind, restart):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(picture(kind)).save(buf, "JPEG", quality=90, subsampling="4:2:0", **({"restart_marker_rows": 1} if restart else {}))
    return buf.getvalue()


def case(kind, restart, n, iters):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from poco_amd import jpeg
    from tests import jpegdec_np
    dev = torch.device("cuda:0")
    data = stream(kind, restart)
    info = jpeg.parse_jpeg(data)
    dec = jpeg.JpegDecoder(dev, H, W, max_batch=n, max_bytes=n * (len(data) + 4096))
    outs = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
    status = torch.empty(n, dtype=torch.int32, device=dev)
    for _ in range(3):
        dec.decode_into([info] * n, outs, status)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert np.array_equal(outs[-1].cpu().numpy(), ref), "device pixels differ from PIL's"
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        dec.decode_into([info] * n, outs, status)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    # the host path: PIL on the pool, then one pinned upload per frame
    pinned = [torch.empty(H, W, 3, dtype=torch.uint8).pin_memory() for _ in range(n)]

    def host(i):
        pinned[i].numpy()[...] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))

    hs = []
    with ThreadPoolExecutor(POOL) as pool:
        for _ in range(max(3, iters // 10)):
            t0 = time.perf_counter()
            list(pool.map(host, range(n)))
            for i in range(n):
                outs[i].copy_(pinned[i], non_blocking=True)
            torch.cuda.synchronize()
            hs.append(1000 * (time.perf_counter() - t0))
    hs.sort()
    return {"bench": "jpeg_decode", "picture": kind, "restart_intervals": len(info.segments), "images": n, "H": H, "W": W,
            "bytes": len(data), "sync_rounds_model": jpegdec_np.sync_rounds(data) if n == 1 else None,
            "gpu_ms_median": round(ms[len(ms) // 2], 4), "gpu_ms_min": round(ms[0], 4), "gpu_ms_max": round(ms[-1], 4),
            "host_pil_upload_ms_median": round(hs[len(hs) // 2], 3), "host_threads": POOL, "iters": iters}


PNG_REPEATS, PNG_POOL = 5, 16


def png_case(source, n):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from poco_amd import png
    dev = torch.device("cuda:0")
    frame = picture("photo")
    if source == "pil":
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, "PNG")
        data = buf.getvalue()
    else:
        data = png.PngEncoder(dev, H, W).encode(torch.from_numpy(frame).to(dev))
    info = png.parse_png(data)
    dec = png.PngDecoder(dev, H, W, max_batch=n, max_bytes=min(1 << 30, n * (len(data) + 4096)))
    outs = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
    status = torch.empty(n, dtype=torch.int32, device=dev)
    dec.decode_into([info] * n, outs, status)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    assert np.array_equal(outs[-1].cpu().numpy(), frame), "device pixels differ from the frame"
    ms = []
    for _ in range(PNG_REPEATS):           # wall time of the call as the demo makes it: bytes in, pixels on the device
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.decode_into([info] * n, outs, status)
        torch.cuda.synchronize()
        ms.append(1000 * (time.perf_counter() - t0))
    pinned = [torch.empty(H, W, 3, dtype=torch.uint8).pin_memory() for _ in range(n)]

    def host(i):
        pinned[i].numpy()[...] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))

    hs = []
    with ThreadPoolExecutor(PNG_POOL) as pool:
        list(pool.map(host, range(n)))
        for _ in range(PNG_REPEATS):
            t0 = time.perf_counter()
            list(pool.map(host, range(n)))
            for i in range(n):
                outs[i].copy_(pinned[i], non_blocking=True)
            torch.cuda.synchronize()
            hs.append(1000 * (time.perf_counter() - t0))
    return {"bench": "png_decode", "source": source, "images": n, "H": H, "W": W, "bytes": len(data),
            "gpu_ms": [round(v, 3) for v in ms], "host_pil_upload_ms": [round(v, 3) for v in hs], "host_threads": PNG_POOL,
            "gpu_worst_below_host_best": max(ms) < min(hs)}


def prog_case(n):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from poco_amd import jpeg
    dev = torch.device("cuda:0")
    data = prog_stream()
    info = jpeg.parse_progressive_jpeg(data)
    dec = jpeg.ProgressiveJpegDecoder(dev, H, W, max_batch=n, max_bytes=n * (len(data) + 4096))
    outs = [torch.empty(H, W, 3, dtype=torch.uint8, device=dev) for _ in range(n)]
    status = torch.empty(n, dtype=torch.int32, device=dev)
    dec.decode_into([info] * n, outs, status)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert np.array_equal(outs[-1].cpu().numpy(), ref), "device pixels differ from PIL's"
    ms = []
    for _ in range(PNG_REPEATS):           # wall time of the call as the demo makes it: bytes in, pixels on the device
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.decode_into([info] * n, outs, status)
        torch.cuda.synchronize()
        ms.append(1000 * (time.perf_counter() - t0))
    pinned = [torch.empty(H, W, 3, dtype=torch.uint8).pin_memory() for _ in range(n)]

    def host(i):
        pinned[i].numpy()[...] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))

    hs = []
    with ThreadPoolExecutor(PNG_POOL) as pool:
        list(pool.map(host, range(n)))
        for _ in range(PNG_REPEATS):
            t0 = time.perf_counter()
            list(pool.map(host, range(n)))
            for i in range(n):
                outs[i].copy_(pinned[i], non_blocking=True)
            torch.cuda.synchronize()
            hs.append(1000 * (time.perf_counter() - t0))
    return {"bench": "jpeg_progressive_decode", "images": n, "H": H, "W": W, "bytes": len(data), "scans": len(info.scans),
            "gpu_ms": [round(v, 3) for v in ms], "host_pil_upload_ms": [round(v, 3) for v in hs], "host_threads": PNG_POOL,
            "gpu_worst_below_host_best": max(ms) < min(hs)}


def prog_stream():
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(picture("photo")).save(buf, "JPEG", quality=90, subsampling="4:2:0", progressive=True)
    return buf.getvalue()


def folder(n, png=False, progressive=False):
    import torch
    import demo
    from poco_amd import synth
    from poco_amd.tester import POCOTester
    from tests import util
    tmp = Path(tempfile.mkdtemp(prefix="poco_decode_"))
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "ckpt.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    imgs = tmp / "imgs"
    imgs.mkdir()
    if png:
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(picture("photo")).save(buf, "PNG")
        data = buf.getvalue()
    elif progressive:
        data = prog_stream()
    else:
        data = stream("photo", False)
    for i in range(n):
        (imgs / (f"im{i:05d}.png" if png else f"im{i:05d}.jpg")).write_bytes(data)
    out = []
    for mode in ("host", "gpu"):
        a = demo.parse_args(["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "ckpt.pt"), "--mode", "folder",
                             "--image_folder", str(imgs), "--output_folder", str(tmp / "out"), "--batch_size", "16",
                             "--smpl", str(tmp / "smpl.npz"), "--decode_png" if png else "--decode_progressive" if progressive else "--decode", mode])
        t = POCOTester(a)
        t.run_on_image_folder(str(imgs), None, str(tmp / "out"))          # warm-up (allocator, file cache)
        st = t.run_on_image_folder(str(imgs), None, str(tmp / "out"))
        out.append({"bench": "folder_decode_png" if png else "folder_decode_progressive" if progressive else "folder_decode", "images": n, "H": H, "W": W, "decode": mode,
                    "ms_per_image": round(1000 * st["seconds"] / n, 2)})
        del t
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--folder", type=int, default=0)
    ap.add_argument("--png", action="store_true", help="the PNG decoder's cases instead of the JPEG decoder's")
    ap.add_argument("--progressive", action="store_true", help="the progressive JPEG decoder's cases instead")
    ap.add_argument("--case", default=None, help="(internal) kind,restart,n | folder,N: run one case in this process")
    ap.add_argument("--limit", type=int, default=240, help="seconds per case")
    args = ap.parse_args()
    if args.case:
        parts = args.case.split(",")
        if parts[0] == "png":
            res = [png_case(parts[1], int(parts[2]))]
        elif parts[0] == "prog":
            res = [prog_case(int(parts[1]))]
        elif parts[0] in ("folder", "pngfolder", "progfolder"):
            res = folder(int(parts[1]), png=parts[0] == "pngfolder", progressive=parts[0] == "progfolder")
        else:
            res = [case(parts[0], parts[1] == "1", int(parts[2]), args.iters)]
        for r in res:
            print(json.dumps(r), flush=True)
        sys.exit(0)
    cases = [f"{k},{r},{n}" for k in ("photo", "noise") for r in (0, 1) for n in (1, 16, 64)]
    if args.png:
        cases = [f"png,{src},{n}" for src in ("pil", "own") for n in (1, 16, 64)]
    if args.progressive:
        cases = [f"prog,{n}" for n in (1, 16, 64)]
    if args.folder:
        cases.append(f"{'pngfolder' if args.png else 'progfolder' if args.progressive else 'folder'},{args.folder}")
    prof = ROOT / "profiles" / ("decode_png.txt" if args.png else "decode_progressive.txt" if args.progressive else "decode.txt")
    prof.parent.mkdir(exist_ok=True)
    with open(prof, "a") as log:
        for c in cases:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, str(Path(__file__).resolve()), "--case", c, "--iters", str(args.iters)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:          # a fault, an abort or the time limit: nothing more is started on the GPU
                msg = json.dumps({"bench": "png_decode" if args.png else "jpeg_progressive_decode" if args.progressive else "jpeg_decode", "case": c, "failed": p.returncode, "stderr": p.stderr[-400:]})
                print(msg, flush=True)
                print(msg, file=log, flush=True)
                sys.exit(1)
            for ln in p.stdout.splitlines():
                if ln.startswith("{"):
                    print(ln, flush=True)
                    print(ln, file=log, flush=True)
