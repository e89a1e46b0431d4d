"""Time the demo renderer (poco_renderer_render: memset + vertex, raster and shade launches) with HIP events at 1920 x 1080 for
1, 4 and 16 SMPL-sized meshes (6890 vertices, 13776 faces, procedurally generated: a deformed torus grid), one JSON line per case.

    python tools/bench_render.py [--iters 50] [--folder 32] [--encode] [--wireframe]
--wireframe: next to each filled call, the wireframe call (poco_renderer_render_ex with POCO_RENDER_WIREFRAME) on the same meshes,
and the keypoint stamp (poco_renderer_draw_discs) of 49 points per person.
--folder N: also the folder-mode wall time per image of demo.py on N synthetic 1080p images (one person each, resnet50-cliff
synthetic checkpoint) without and with --render (PNG encoding on the host included).
--encode: instead of the renderer, the JPEG encoder (poco_jpeg_encode: transform, entropy, compaction) at 1920 x 1080 and at
3840 x 1080 (--sideview) on a rendered frame and on a noise frame, device events around each call, median of --iters; with
--folder N the folder-mode wall time per image without --render and with --render as png and as jpg, without and with --sideview.
The PNG encoder (poco_png_encode) follows on the same frames, beside the host path it replaces (D2H copy + PIL to memory on one
thread) and PIL's size, and with --folder N the wall time per image of --render --encode host and --encode gpu, 5 repeats each."""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from poco_amd import render  # noqa: E402

V_SMPL, F_SMPL = 6890, 13776


def smpl_sized_mesh():
    """A closed 65 x 106 torus grid (6890 vertices, 13780 triangles, 4 dropped -> 13776) squashed into a body-sized shape."""
    n, m = 106, 65
    u = np.linspace(0, 2 * np.pi, n, endpoint=False)
    v = np.linspace(0, 2 * np.pi, m, endpoint=False)
    U, Vv = np.meshgrid(u, v, indexing="ij")
    x = (0.25 + 0.08 * np.cos(Vv)) * np.cos(U)
    z = (0.25 + 0.08 * np.cos(Vv)) * np.sin(U) * 0.6
    y = 0.08 * np.sin(Vv) + 0.9 * np.sin(U / 2) ** 2 - 0.45
    verts = np.stack([x, y * 2.0, z], -1).reshape(-1, 3).astype(np.float32)
    faces = []
    for i in range(n):
        for j in range(m):
            a, b, c, d = i * m + j, ((i + 1) % n) * m + j, i * m + (j + 1) % m, ((i + 1) % n) * m + (j + 1) % m
            faces += [(a, b, d), (a, d, c)]
    faces = np.array(faces[:F_SMPL], np.int32)
    assert verts.shape[0] == V_SMPL and faces.shape[0] == F_SMPL
    return verts, faces


def people(P, H, W, verts, seed=0):
    """P copies spread over the frame (a grid of cells), each about 0.8 of its cell tall, slightly rotated per person."""
    r = np.random.default_rng(seed)
    g = int(np.ceil(np.sqrt(P)))
    vs, cams = [], []
    for p in range(P):
        a = r.uniform(-0.5, 0.5)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
        vs.append(verts @ R.T)
        s = 0.8 / g
        cx, cy = (p % g + 0.5) / g * 2 - 1, (p // g + 0.5) / g * 2 - 1        # cell centre in NDC
        cams.append([s * H / W, s, cx / (s * H / W), -cy / s])
    return np.stack(vs), np.array(cams, np.float32)


def _time(fn, iters):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def bench(iters, wireframe=False):
    dev = torch.device("cuda:0")
    H, W = 1080, 1920
    verts, faces = smpl_sized_mesh()
    R = render.Renderer(faces, V_SMPL, dev)
    for P in (1, 4, 16):
        vs, cams = people(P, H, W, verts)
        cols = np.array([render.vertex_color(np.full(24, 0.3 + 0.04 * p, np.float32), "hrnet_w48_cls-cliff") for p in range(P)])
        mats = np.zeros(P, np.float32)
        dv = torch.from_numpy(vs).to(dev)
        frame = torch.zeros(H, W, 3, dtype=torch.uint8, device=dev)
        cnt = torch.zeros(H, W, dtype=torch.int32, device=dev)
        R.render(frame, dv, cams, cols, mats, frag_count=cnt)
        frags, covered = int(cnt.sum()), int((cnt > 0).sum())
        for _ in range(5):
            R.render(frame, dv, cams, cols, mats)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            R.render(frame, dv, cams, cols, mats)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        print(json.dumps({"bench": "render", "H": H, "W": W, "people": P, "verts": V_SMPL, "faces": F_SMPL, "fragments": frags,
                          "covered_px": covered, "ms": round(ms, 4), "iters": iters}), flush=True)
        if wireframe:
            R.render(frame, dv, cams, cols, mats, frag_count=cnt, wireframe=True)
            frags, covered = int(cnt.sum()), int((cnt > 0).sum())
            ms = _time(lambda: R.render(frame, dv, cams, cols, mats, wireframe=True), iters)
            print(json.dumps({"bench": "render_wireframe", "H": H, "W": W, "people": P, "verts": V_SMPL, "faces": F_SMPL,
                              "fragments": frags, "covered_px": covered, "ms": round(ms, 4), "iters": iters}), flush=True)
            r = np.random.default_rng(P)
            pts = torch.from_numpy(r.uniform([0, 0], [W, H], (49 * P, 2)).astype(np.float32)).to(dev)
            rgb = torch.full((49 * P, 3), 255, dtype=torch.uint8, device=dev)
            ms = _time(lambda: render.draw_discs(frame, pts, rgb), iters)
            print(json.dumps({"bench": "draw_discs", "H": H, "W": W, "points": 49 * P, "radius": render.DISC_RADIUS,
                              "ms": round(ms, 4), "iters": iters}), flush=True)


def encode(iters):
    """One encode call (three launches, no host sync inside the timed window) per frame kind and size; also the bytes it makes."""
    from poco_amd import jpeg
    dev = torch.device("cuda:0")
    H, W = 1080, 1920
    verts, faces = smpl_sized_mesh()
    R = render.Renderer(faces, V_SMPL, dev)
    vs, cams = people(4, H, W, verts)
    cols = np.array([render.vertex_color(np.full(24, 0.3 + 0.04 * p, np.float32), "hrnet_w48_cls-cliff") for p in range(4)])
    g = torch.linspace(0, 255, W, device=dev)[None, :, None] * torch.tensor([1.0, 0.6, 0.3], device=dev)
    smooth = (g + torch.linspace(0, 60, H, device=dev)[:, None, None]).clamp(0, 255).to(torch.uint8).contiguous()
    rendered = render.render_people(R, smooth.clone(), torch.from_numpy(vs).to(dev), cams, None, "hrnet_w48_cls-cliff",
                                    uncert_color=False, sideview=True, side_bg=255).contiguous()
    R.render(smooth, torch.from_numpy(vs).to(dev), cams, cols, np.zeros(4, np.float32))
    noise = torch.randint(0, 256, (H, 2 * W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(0))
    enc = jpeg.JpegEncoder(dev, H, 2 * W)
    out = torch.empty(jpeg.worst_case_bytes(H, 2 * W), dtype=torch.uint8, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    for kind, w, frame in (("rendered", W, smooth), ("rendered", 2 * W, rendered), ("noise", W, noise[:, :W].contiguous()),
                           ("noise", 2 * W, noise)):
        for q in (90,):
            for _ in range(5):
                enc.encode_into(frame, out, q, n)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
            for e0, e1 in ev:
                e0.record()
                enc.encode_into(frame, out, q, n)
                e1.record()
            torch.cuda.synchronize()
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
            print(json.dumps({"bench": "jpeg_encode", "frame": kind, "H": H, "W": w, "quality": q, "bytes": int(n.item()),
                              "ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                              "iters": iters}), flush=True)
    # the PNG encoder on the same frames: the encode call (device events), the host path it replaces (D2H copy + PIL's encoder to
    # memory, one thread, median of 5) and the two sizes
    import io
    import time
    from PIL import Image
    from poco_amd import png
    penc = png.PngEncoder(dev, H, 2 * W)
    pout = torch.empty(png.worst_case_bytes(H, 2 * W), dtype=torch.uint8, device=dev)
    for kind, w, frame in (("rendered", W, smooth), ("rendered", 2 * W, rendered), ("noise", W, noise[:, :W].contiguous()),
                           ("noise", 2 * W, noise)):
        for _ in range(5):
            penc.encode_into(frame, pout, n)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in ev:
            e0.record()
            penc.encode_into(frame, pout, n)
            e1.record()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        host = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            buf = io.BytesIO()
            Image.fromarray(frame.cpu().numpy()).save(buf, "PNG")
            host.append(1000 * (time.perf_counter() - t0))
        print(json.dumps({"bench": "png_encode", "frame": kind, "H": H, "W": w, "bytes": int(n.item()), "pil_bytes": buf.tell(),
                          "ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                          "host_d2h_pil_ms_median": round(sorted(host)[2], 2), "iters": iters}), flush=True)


def folder(n, flag_sets=([], ["--render"], ["--render", "--sideview"]), repeats=1):
    import demo
    from PIL import Image
    from poco_amd import synth
    from tests import util
    tmp = Path(tempfile.mkdtemp(prefix="poco_render_"))
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "ckpt.pt")
    smpl = synth.synth_smpl(7)
    smpl["faces"] = smpl_sized_mesh()[1]
    np.savez(tmp / "smpl.npz", **smpl)
    imgs = tmp / "imgs"
    imgs.mkdir()
    r = np.random.default_rng(0)
    for i in range(n):
        Image.fromarray(r.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)).save(imgs / f"im{i:05d}.png")
    from poco_amd.tester import POCOTester
    for extra in flag_sets:
        a = demo.parse_args(["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "ckpt.pt"), "--mode", "folder",
                             "--image_folder", str(imgs), "--output_folder", str(tmp / "out"), "--batch_size", "16",
                             "--smpl", str(tmp / "smpl.npz"), *extra])
        t = POCOTester(a)
        t.run_on_image_folder(str(imgs), None, str(tmp / "out"))          # warm-up (allocator, file cache)
        runs = [1000 * t.run_on_image_folder(str(imgs), None, str(tmp / "out"))["seconds"] / n for _ in range(repeats)]
        rec = {"bench": "folder_render", "images": n, "H": 1080, "W": 1920, "flags": " ".join(extra) or "(none)",
               "ms_per_image": round(sorted(runs)[len(runs) // 2], 2)}
        if repeats > 1:
            rec.update(repeats=repeats, ms_per_image_min=round(min(runs), 2), ms_per_image_max=round(max(runs), 2))
        print(json.dumps(rec), flush=True)
        del t


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--folder", type=int, default=0)
    ap.add_argument("--encode", action="store_true")
    ap.add_argument("--wireframe", action="store_true")
    args = ap.parse_args()
    if args.encode:
        encode(args.iters)
        if args.folder:
            jpg = ["--image_format", "jpg"]
            folder(args.folder, ([], ["--render"], ["--render", *jpg], ["--render", "--sideview"], ["--render", "--sideview", *jpg]))
            # the PNG path on the host against the PNG path on the device: 5 repeats each, the spread is reported
            folder(args.folder, (["--render", "--encode", "host"], ["--render", "--encode", "gpu"]), repeats=5)
    else:
        bench(args.iters, args.wireframe)
        if args.folder:
            folder(args.folder)
