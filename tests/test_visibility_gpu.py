"""GPU: poco_op_part_visibility (csrc/part_visibility.hip) against the numpy restatement tests/visibility_np.py, by INTEGER EQUALITY:
hand-made meshes of 2 to 12 faces (occlusion fully and half, frame edge / margin / outside the window, a shared edge through pixel
centres, coincident front and back faces, the degenerate faces, equal depth) at res 17, 32, 33 x margin 0, 8, res x B 1, 3, under four
masks; a 642-vertex sphere of 24 parts at res 224; `front` against the label counts of ops.part_labels on every case; pre-filled
outputs, guard bands around output and scratch, two runs; and poco_dataset_crop_occ_mask against the restatement's alpha > 0 map."""
import numpy as np
import pytest
import torch

from poco_amd import datacrop, ops
from tests import datacrop_cases, occlude_cases, occlude_np, visibility_np

pytestmark = pytest.mark.gpu
PATTERN = 0x5A5AA5A5
RES = [17, 32, 33]


def _margins(res):
    return [0, 8, res]


def hand_meshes(res):
    """name -> visibility_np.Mesh; coordinates in multiples of 1/8 pixel, built around the frame's size so every res has the same cases."""
    h = res // 2
    out = {}
    # a) part 1 fully in front of part 2, then half in front
    for name, x1 in (("front_full", 2 * h - 1), ("front_half", h)):
        m = visibility_np.Mesh(res)
        a, b, c, d = m.vert(1, 1, 96.0), m.vert(2 * h - 1, 1, 96.0), m.vert(2 * h - 1, 5, 96.0), m.vert(1, 5, 96.0)
        m.tri(a, b, c, 2); m.tri(a, c, d, 2)
        a, b, c, d = m.vert(1, 1), m.vert(x1, 1), m.vert(x1, 5), m.vert(1, 5)
        m.tri(a, b, c, 1); m.tri(a, c, d, 1)
        out[name] = m
    # b) straddling the frame's right edge, wholly in the margin (4 px beyond the frame), wholly outside every window (beyond 2 res)
    m = visibility_np.Mesh(res)
    m.tri((res - 3.25, 2.25), (res + 3.25, 2.25), (res - 3.25, 8.75), 3)
    m.tri((-6.75, 3.25), (-1.25, 3.25), (-6.75, 9.25), 4)
    m.tri((3 * res, 3 * res), (3 * res + 6, 3 * res), (3 * res, 3 * res + 6), 5)
    m.tri((2.25, res + 1.25), (9.75, res + 1.25), (2.25, res + 6.75), 23)
    out["edges"] = m
    # c) two faces of one part sharing the diagonal through pixel centres; d) front and back face coincident in the image
    m = visibility_np.Mesh(res)
    a, b, c, d = m.vert(2, 2), m.vert(10, 2), m.vert(10, 10), m.vert(2, 10)
    m.tri(a, b, c, 6); m.tri(a, c, d, 6)
    m.tri((2.5, 11.5), (12.5, 11.5), (2.5, 15.5), 7)
    m.tri((2.5, 11.5, 128.0), (2.5, 15.5, 128.0), (12.5, 11.5, 128.0), 7)
    out["shared_and_coincident"] = m
    # e) degenerate faces beside one good face; f) equal depth between parts 10 and 11: the lower face index wins
    m = visibility_np.Mesh(res)
    m.tri((0.25, 0.25), (6.25, 0.25), (0.25, 6.25), 10)
    m.tri((0.25, 0.25), (6.25, 0.25), (0.25, 6.25), 11)
    m.tri((0, 0), (res, 0), (h, res, 0.05), 12)
    m.tri((0, 0), (res, 0), (float("nan"), res), 13)
    m.tri((1, 1), (3, 3), (5, 5), 14)
    m.tri((8.25, 8.25), (14.25, 8.25), (8.25, 14.25), 15)
    out["degenerate_and_ties"] = m
    return out


def _world(res, B):
    """All hand meshes of one res as ONE list of (verts [B,V,3], cam_t [B,3], faces, parts): crop 0 sees the mesh as built, crops 1 and 2
    from cameras moved by fractions of a pixel and nearer / farther, where nothing is exact any more."""
    cams = np.array([[0, 0, 0], [0.013, -0.021, 3.0], [-0.37, 0.11, -9.0]], np.float32)[:B]
    worlds = {}
    for name, m in hand_meshes(res).items():
        assert m.exact(), name
        v, f, p = m.arrays()
        if name == "degenerate_and_ties":
            f = np.concatenate([f, [[0, 0, 1], [0, 1, 999], [-1, 0, 1]]]).astype(np.int32)       # a repeated and two bad indices
            p = np.concatenate([p, [16, 17, 18]]).astype(np.uint8)
        assert 2 <= len(f) <= 12
        worlds[name] = (np.repeat(v[None], B, 0), cams, f, p, m.focal)
    return worlds


def _masks(res, B):
    chk = ((np.add.outer(np.arange(res), np.arange(res)) % 2) == 0).astype(np.uint8)
    return {"null": None, "zeros": np.zeros((B, res, res), np.uint8), "ones": np.full((B, res, res), 255, np.uint8),
            "checker": np.repeat(chk[None], B, 0)}


def _dev(cuda, v, t, f, p):
    return (torch.from_numpy(v).to(cuda), torch.from_numpy(t).to(cuda), torch.from_numpy(f).to(cuda), torch.from_numpy(p).to(cuda))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("res", RES)
def test_hand_meshes_equal_the_restatement(cuda, res, B):
    for name, (v, t, f, p, focal) in _world(res, B).items():
        dv, dt, df, dp = _dev(cuda, v, t, f, p)
        labels = ops.part_labels(dv, dt, df, dp, focal, res).cpu().numpy()
        for margin in _margins(res):
            want = {k: visibility_np.part_visibility(v, t, f, p, focal, res, margin, mk) for k, mk in _masks(res, B).items()}
            for k, mk in _masks(res, B).items():
                dm = None if mk is None else torch.from_numpy(mk).to(cuda)
                out = torch.full((B, 24, 4), PATTERN, dtype=torch.int32, device=cuda)            # every word must be overwritten
                got = ops.part_visibility(dv, dt, df, dp, focal, res, margin, dm, out=out, h_face_part=p).cpu().numpy()
                assert np.array_equal(got, want[k]), (name, margin, k, np.argwhere(got != want[k])[:4])
                for q in range(24):                                                              # front = the label counts
                    assert (got[:, q, 2] == (labels == q + 1).reshape(B, -1).sum(1)).all(), (name, margin, k, q)
                assert (got[:, :, 3] <= got[:, :, 2]).all() and (got[:, :, 2] <= got[:, :, 1]).all() and (got[:, :, 1] <= got[:, :, 0]).all()
            assert np.array_equal(want["null"], want["zeros"]) and not want["ones"][:, :, 3].any()
            assert np.array_equal(want["ones"][:, :, :3], want["null"][:, :, :3])
            assert (want["checker"][:, :, 3] <= want["null"][:, :, 3]).all()
            c = want["null"][0]                                                                  # crop 0: the mesh as built
            if name == "front_full":
                assert c[2, 2] == 0 and c[2, 1] == c[2, 0] > 0 and c[1, 2] == c[1, 1] == c[2, 1]
            if name == "front_half":
                assert 0 < c[2, 2] and c[2, 2] + c[1, 2] == c[2, 1] and 2 * c[2, 2] == c[2, 1]
            if name == "edges":
                assert not c[5].any() and 0 < c[3, 1] and c[3, 1] == c[3, 2]
                assert (c[3, 0] > c[3, 1]) == (margin > 0) and (c[4, 0] > 0) == (margin > 0) and c[4, 1] == 0
                assert (c[23, 0] > 0) == (margin > 0) and c[23, 1] == 0
            if name == "shared_and_coincident":
                assert c[6].tolist() == [64, 64, 64, 64]                                         # [2, 10]^2: 8 x 8 centres, each once
                assert c[7, 0] == c[7, 1] == c[7, 2] > 0
            if name == "degenerate_and_ties":
                assert c[10].tolist() == [21, 21, 21, 21] and c[11].tolist() == [21, 21, 0, 0] and c[15, 0] == 21
                assert not c[[12, 13, 14, 16, 17, 18]].any()


def test_sphere_of_24_parts_at_full_size(cuda):
    v, f, p = visibility_np.sphere(3)
    assert v.shape == (642, 3) and f.shape == (1280, 3) and sorted(set(p.tolist())) == list(range(24))
    verts = np.repeat(v[None], 2, 0)
    cam_t = np.array([[0.02, -0.01, 23.0], [0.9, 0.35, 30.0]], np.float32)                       # wider than the crop; off to a corner
    r = np.random.default_rng(4)
    mask = (r.random((2, 224, 224)) < 0.3).astype(np.uint8)
    want = visibility_np.part_visibility(verts, cam_t, f, p, 5000.0, 224, 112, mask)
    dv, dt, df, dp = _dev(cuda, verts, cam_t, f, p)
    got = ops.part_visibility(dv, dt, df, dp, 5000.0, 224, 112, torch.from_numpy(mask).to(cuda)).cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:6]
    assert (want[:, :, 0] > 0).all() and (want[0, :, 0] > want[0, :, 1]).any() and (want[:, :, 2] < want[:, :, 1]).any()
    assert (want[:, :, 3] < want[:, :, 2]).any()
    labels = ops.part_labels(dv, dt, df, dp, 5000.0, 224).cpu().numpy()
    assert np.array_equal(got[:, :, 2], np.stack([(labels == q + 1).reshape(2, -1).sum(1) for q in range(24)], 1))
    # a part table above 23 is refused with the host copy, clamped without it
    bad = p.copy()
    bad[::7] = 200
    with pytest.raises(Exception, match="has part 200"):
        ops.part_visibility(dv, dt, df, torch.from_numpy(bad).to(cuda), 5000.0, 224, 112, h_face_part=bad)
    clamped = ops.part_visibility(dv, dt, df, torch.from_numpy(bad).to(cuda), 5000.0, 224, 112).cpu().numpy()
    assert np.array_equal(clamped, visibility_np.part_visibility(verts, cam_t, f, np.minimum(bad, 23), 5000.0, 224, 112))


def test_guard_bands_and_repeatability(cuda):
    """Output and scratch sit inside larger allocations filled with a bit pattern: nothing outside them changes; two runs give equal
    bits; a scratch that is too small is refused."""
    res, margin, B = 33, 8, 3
    v, t, f, p, focal = _world(res, B)["edges"]
    dv, dt, df, dp = _dev(cuda, v, t, f, p)
    nbytes = ops.part_visibility_scratch_bytes(B, res, margin)
    assert nbytes == B * (res * res * 8 + 49 * 49 * 4)
    G = 4096
    big_out = torch.full((G + B * 96 + G,), PATTERN, dtype=torch.int32, device=cuda)
    big_scr = torch.full((G + nbytes + G,), 0xA5, dtype=torch.uint8, device=cuda)
    out = big_out[G:G + B * 96].view(B, 24, 4)
    runs = []
    for _ in range(2):
        ops.part_visibility(dv, dt, df, dp, focal, res, margin, out=out, scratch=big_scr[G:G + nbytes])
        runs.append(out.cpu().numpy().copy())
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], visibility_np.part_visibility(v, t, f, p, focal, res, margin))
    assert bool((big_out[:G] == PATTERN).all()) and bool((big_out[G + B * 96:] == PATTERN).all())
    assert bool((big_scr[:G] == 0xA5).all()) and bool((big_scr[G + nbytes:] == 0xA5).all())
    with pytest.raises(Exception, match="scratch"):
        ops.part_visibility(dv, dt, df, dp, focal, res, margin, scratch=big_scr[G:G + nbytes - 8])
    with pytest.raises(Exception, match="margin"):
        ops.part_visibility(dv, dt, df, dp, focal, res, res + 1)


# ---- the occluder mask out of the dataset crop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [32, 224])
def test_crop_mask_equals_the_alpha_map_and_leaves_crops_and_cover_alone(cuda, res):
    from tests.test_occlude_gpu import _columns
    imgs, cuts = datacrop_cases.images(), occlude_cases.cutouts()
    dimgs, atlas = [torch.from_numpy(i).to(cuda) for i in imgs], datacrop.OccluderAtlas(cuts, cuda)
    g = occlude_cases.geometry(res)
    names = list(g)
    objects = [g[k] for k in names]
    c = _columns(len(objects))
    params = datacrop.batch_params(c["center"], c["scale"], c["rot"], c["flip"], c["pn"], np.ones(len(objects)), res)
    occ = (atlas, datacrop.occ_records(objects))
    crops0, cover0 = datacrop.dataset_crop(dimgs, c["img"], params, res, True, occlusion=occ)
    crops, cover, mask = datacrop.dataset_crop(dimgs, c["img"], params, res, True, occlusion=occ, want_mask=True)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (len(objects), res, res)
    mask = mask.cpu().numpy()
    zero = np.zeros((res, res, 3), np.float32)
    for n, name in enumerate(names):
        want = occlude_np.apply_objects_np(zero, cuts, objects[n])[1]
        assert np.array_equal(mask[n], want.astype(np.uint8)), name
    assert np.array_equal(mask.reshape(len(objects), -1).sum(1), cover.cpu().numpy())            # the cells count the mask's pixels
    assert np.array_equal(cover.cpu().numpy(), cover0.cpu().numpy())
    assert np.array_equal(crops.cpu().numpy().view(np.uint32), crops0.cpu().numpy().view(np.uint32))
    assert mask[names.index("none")].sum() == 0 and mask[names.index("seven")].sum() > 0
