"""Inputs of tests/test_crop_seam_*.py: batches of N = 65 535 + 5 crops for the five host loops that split a batch at the gridDim.y / z
limit (launch_crop_t, launch_crop_normalize_multi, poco_dataset_crop, crop_occ_entry, poco_op_corrupt), their restatements at the rows
around the seam, and poisoned guard-banded device buffers.

Every crop's input is a deterministic function of its index n, built vectorised (a Python loop over 65 540 records would dominate the
test), chosen so that
  * crops n and n + 65 535 differ (an offset that wraps to the start of the batch shows),
  * neighbouring crops differ (an offset that is one record short shows),
  * every per-crop array has a stride of its own at res = 4: boxes 16 or 32 bytes, frame_idx 4, records 48, occluder records 144,
    cover 4, mask 16, steps 56 (chain_len = 2), out 192 bytes.
The restatements (oracle/crop_np.py, tests/datacrop_np.py, tests/occlude_np.py, tests/corrupt_np.py) are evaluated at REF_ROWS only:
crops 0..4, 65 531..65 539 (the last two of the batch among them); they are far too slow for all N."""
import functools

import numpy as np

from oracle import crop_np
from tests import corrupt_np, datacrop_np, occlude_np

LIMIT = 65535                       # gridDim.y / gridDim.z limit: the chunk of the five host loops
N = LIMIT + 5
SPLIT = 40000                       # the two-call comparison: [0, SPLIT) and [SPLIT, N), each below LIMIT
RES = 4
REF_ROWS = np.array(list(range(0, 5)) + list(range(LIMIT - 4, N)))            # 0..4, 65531..65539
SEAM_ROWS = list(range(LIMIT - 2, N))                                          # 65533..65539: pairwise different, and from 0..4
GUARD = 4096                        # elements of poison before and after a buffer
assert SPLIT < LIMIT and N - SPLIT < LIMIT and N - 1 == REF_ROWS[-1]


def idx():
    return np.arange(N, dtype=np.int64)


# ---- the inference crop ----------------------------------------------------------------------------------------------------------
CROP_HW = (37, 53)
N_FRAMES = 7


@functools.lru_cache(None)
def crop_frames():
    r = np.random.default_rng(77)
    return [r.integers(0, 256, CROP_HW + (3,), dtype=np.uint8) for _ in range(N_FRAMES)]


def crop_boxes(dtype):
    """[N,4] (cx, cy, w, h): centres on a 43 x 31 lattice with fractions, sides in 6..20; the +1.5 on w past the seam keeps crop
    n + 65 535 from repeating crop n.  The tenths are not float32 numbers, so the float64 boxes are not the float32 ones."""
    n = idx().astype(np.float64)
    cx = 4.0 + (n * 7) % 43 + 0.1 * (n % 5)
    cy = 3.0 + (n * 11) % 31 + 0.5 * (n % 3)
    w = 6.0 + n % 13 + 1.5 * (n // LIMIT)
    h = 5.0 + (n * 3) % 17
    return np.ascontiguousarray(np.stack([cx, cy, w, h], 1).astype(dtype))


def frame_index():
    """int32 [N]: not periodic in 65 535 - (n + n // 11) % 7 moves by 1 or 2 (mod 7) from n to n + 65 535."""
    n = idx()
    f = ((n + n // 11) % N_FRAMES).astype(np.int32)
    assert (f[LIMIT:] != f[:N - LIMIT]).all() and len(set(f[SEAM_ROWS].tolist())) > 2
    return f


@functools.lru_cache(None)
def crop_reference(kind, scale=1.1):
    """The restatement at REF_ROWS: kind 'f32', 'f64' (frame 0) or 'multi' (frame frame_index()[n]).  float32 [14,3,RES,RES]."""
    boxes = crop_boxes(np.float64 if kind == "f64" else np.float32)
    fidx = frame_index() if kind == "multi" else np.zeros(N, np.int32)
    frames = crop_frames()
    out = np.concatenate([crop_np.crop_normalize_np(frames[fidx[n]], boxes[n:n + 1], scale, RES) for n in REF_ROWS])
    out.setflags(write=False)
    return out


# ---- the dataset crop ------------------------------------------------------------------------------------------------------------
DC_SIZES = ((23, 31), (17, 40), (29, 19))
DC_ROTS = (0.0, 20.0, -35.0)


@functools.lru_cache(None)
def dc_images():
    r = np.random.default_rng(78)
    return [r.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in DC_SIZES]


@functools.lru_cache(None)
def dc_inputs():
    """dict of per-crop arrays: img, cx, cy, bb (box side in pixels), rot (degrees), flip, pn [N,3]."""
    n = idx()
    d = dict(img=((n + n // 13) % 3).astype(np.int32), cx=2 + (n * 5) % 29, cy=1 + (n * 3) % 23, bb=6 + n % 11 + 2 * (n // LIMIT),
             rot=np.asarray(DC_ROTS)[n % 3], flip=((n // 2) % 2).astype(np.int32),
             pn=1.0 + (((n[:, None] * np.array([1, 2, 3])) % 7) - 3) * 0.05)
    assert (d["img"][LIMIT:] != d["img"][:N - LIMIT]).all()
    return d


def dc_params():
    """datacrop.PARAM_DTYPE [N]: datacrop.crop_params for every crop, vectorised (the rotation's sin / cos are taken per distinct
    angle with the scalar calls crop_params makes; the products and roundings are IEEE operations, the same in an array)."""
    from poco_amd import datacrop
    d = dc_inputs()
    half = (d["bb"] * 1.0 * 0.5).astype(np.float32).astype(np.float64)
    sn = np.array([np.float64(np.sin(np.pi * r / 180)) for r in DC_ROTS])[idx() % 3]
    cs = np.array([np.float64(np.cos(np.pi * r / 180)) for r in DC_ROTS])[idx() % 3]
    zero = np.zeros(N)
    down = ((zero * cs - half * sn).astype(np.float32), (zero * sn + half * cs).astype(np.float32))
    right = ((half * cs - zero * sn).astype(np.float32), (half * sn + zero * cs).astype(np.float32))
    cx, cy = d["cx"].astype(np.float64), d["cy"].astype(np.float64)
    rec = np.zeros(N, datacrop.PARAM_DTYPE)
    rec["img"], rec["flip"], rec["pn"], rec["bb"] = d["img"], d["flip"], d["pn"], d["bb"]
    rec["src"] = np.stack([cx, cy, cx + down[0].astype(np.float64), cy + down[1].astype(np.float64), cx + right[0].astype(np.float64),
                           cy + right[1].astype(np.float64)], 1)
    for n in REF_ROWS:                                    # the vectorised records are crop_params' records
        one = datacrop.crop_params((d["cx"][n], d["cy"][n]), d["bb"][n] / 200.0, d["rot"][n], d["flip"][n], d["pn"][n], 1.0, RES)
        one["img"] = d["img"][n]
        assert one.tobytes() == rec[n].tobytes(), n
    return rec


@functools.lru_cache(None)
def occluders():
    """three small RGBA cut-outs; a third of the alphas 0, a fifth 255"""
    r = np.random.default_rng(79)
    cut = []
    for h, w in ((5, 4), (6, 6), (3, 7)):
        a = r.integers(0, 256, (h, w, 4), dtype=np.uint8)
        u = r.uniform(size=(h, w))
        a[..., 3] = np.where(u < 0.33, 0, np.where(u > 0.8, 255, a[..., 3]))
        cut.append(a)
    return cut


def occ_records():
    """datacrop.OCC_DTYPE [N]: 1 or 2 objects per crop, every field a function of n, sizes within the cut-out's (INTER_AREA only)."""
    from poco_amd import datacrop
    n = idx()
    hw = np.array([a.shape[:2] for a in occluders()])
    rec = np.zeros(N, datacrop.OCC_DTYPE)
    rec["count"] = 1 + n % 2
    for k in range(2):
        oid = (n + k) % 3
        rec["obj"]["id"][:, k] = oid
        rec["obj"]["dst_w"][:, k] = 1 + (n // 3 + k) % hw[oid, 1]
        rec["obj"]["dst_h"][:, k] = 1 + (n // 5 + k) % hw[oid, 0]
        rec["obj"]["cx"][:, k] = (n + 2 * k) % 5
        rec["obj"]["cy"][:, k] = (n // 4 + k) % 5
    return rec


def occ_objects(rec, n):
    return [tuple(int(rec["obj"][f][n, k]) for f in ("id", "dst_w", "dst_h", "cx", "cy")) for k in range(int(rec["count"][n]))]


@functools.lru_cache(None)
def dc_reference(occ, normalize):
    """The restatement at REF_ROWS: (out float32 [14,3,RES,RES], mask uint8 [14,RES,RES], cover int32 [14]); without occluders the
    mask and the cover are zero."""
    d, images = dc_inputs(), dc_images()
    rec = occ_records() if occ else None
    outs, masks = [], []
    for n in REF_ROWS:
        img, c, s = images[d["img"][n]], (d["cx"][n], d["cy"][n]), d["bb"][n] / 200.0
        assert datacrop_np.py_round(s * 200.0) == d["bb"][n]
        if not occ:
            outs.append(datacrop_np.rgb_processing_np(img, c, s, d["rot"][n], d["flip"][n], d["pn"][n], RES, normalize))
            masks.append(np.zeros((RES, RES), np.uint8))
            continue
        objs = occ_objects(rec, n)
        o, cover = occlude_np.rgb_processing_occ_np(img, c, s, d["rot"][n], d["flip"][n], d["pn"][n], occluders(), objs, RES, normalize)
        x = datacrop_np.crop_cv2_np(img, c, s, RES, d["rot"][n])
        _, touched = occlude_np.apply_objects_np(np.fliplr(x) if d["flip"][n] else x, occluders(), objs)
        assert int(touched.sum()) == cover
        outs.append(o)
        masks.append(touched.astype(np.uint8))
    out, mask = np.stack(outs), np.stack(masks)
    cover = mask.reshape(len(mask), -1).sum(1).astype(np.int32)
    for a in (out, mask, cover):
        a.setflags(write=False)
    return out, mask, cover


# ---- corrupt ---------------------------------------------------------------------------------------------------------------------
CHAIN = 2
CORRUPT_SEED = (5 << 32) | 1234


def corrupt_input():
    """raw crops float32 [N,3,RES,RES] in [0, 255]: tenths, different in every crop"""
    n = idx()[:, None]
    e = np.arange(3 * RES * RES, dtype=np.int64)[None, :]
    return (((n * 37 + e * 101 + (n // 256) * 13) % 2551) / 10.0).astype(np.float32).reshape(N, 3, RES, RES)


def corrupt_records():
    """ops.CORRUPT_STEP [N, 2], both positions populated.  Position 0 cycles through noise, gamma, contrast, pixelate, both blurs with
    a parameter that depends on n; position 1 is gaussian_noise (gamma after a noise) - so every crop draws noise under a stream of
    its own, n or 100 000 + n, and a step read from another crop's record, or from the other position, changes the result."""
    from poco_amd import ops
    K = ops.CORRUPT_KINDS.index
    n = idx()
    rec = np.zeros((N, CHAIN), ops.CORRUPT_STEP)
    rec["seed"][:, :, 0], rec["seed"][:, :, 1] = CORRUPT_SEED & 0xFFFFFFFF, CORRUPT_SEED >> 32
    m = n % 6
    kind0 = np.array([K("gaussian_noise"), K("gamma"), K("contrast"), K("pixelate"), K("gaussian_blur"), K("motion_blur")])[m]
    rec["kind"][:, 0] = kind0
    rec["p0"][:, 0] = np.select([m == 0, m == 1, m == 2, m == 4, m == 5], [2.0 + n % 9, 0.5 + 0.25 * (n % 7), 0.25 * (n % 8), 0.4 + 0.1 * (n % 5), 0.6], 0.0)
    rec["p1"][:, 0] = np.where(m == 5, 0.8, 0.0)
    rec["ival"][:, 0] = np.select([m == 3, m == 5], [2 + n % 2, 3], 0)
    rec["stream"][:, 0] = n
    rec["kind"][:, 1] = np.where(m == 0, K("gamma"), K("gaussian_noise"))
    rec["p0"][:, 1] = np.where(m == 0, 0.8 + 0.1 * (n % 4), 1.0 + n % 11)
    rec["stream"][:, 1] = 100000 + n
    return rec


@functools.lru_cache(None)
def corrupt_reference(normalize):
    x, rec = corrupt_input()[REF_ROWS], corrupt_records()[REF_ROWS]
    out = corrupt_np.corrupt(x, corrupt_np.chains_from_records(rec), normalize)
    out.setflags(write=False)
    return out


# ---- what every case asserts -----------------------------------------------------------------------------------------------------
def assert_seam_rows_distinct(ref):
    """`ref` = a restatement at REF_ROWS.  Crops 65 533..65 539 differ pairwise and from crops 0..4: an offset that is short, long, or
    wraps to the start of the batch puts a different crop where the test looks."""
    pos = {int(n): i for i, n in enumerate(REF_ROWS)}
    for a in SEAM_ROWS:
        for b in list(range(5)) + SEAM_ROWS:
            if a != b:
                assert not np.array_equal(ref[pos[a]], ref[pos[b]]), (a, b)


class Guarded:
    """A contiguous device tensor of `shape` inside one allocation with GUARD poisoned elements on either side, itself poisoned: the
    poison is ops.POISON_BITS (float32, int32) or 0xA5 (uint8), none of which a crop kernel can store."""

    def __init__(self, shape, dtype, device):
        import torch
        from poco_amd import ops
        self.n = int(np.prod(shape))
        self.flat = torch.empty(self.n + 2 * GUARD, dtype=dtype, device=device)
        if dtype == torch.uint8:
            self.bits, self.poison = self.flat, 0xA5
        else:
            self.bits, self.poison = self.flat.view(torch.int32), ops.POISON_BITS
        self.bits.fill_(self.poison)
        self.body = self.flat[GUARD:GUARD + self.n].view(shape)

    def check(self, what):
        """the guard bands hold the poison, the body holds none of it"""
        g = self.bits
        assert bool((g[:GUARD] == self.poison).all()) and bool((g[GUARD + self.n:] == self.poison).all()), f"{what}: a guard band was written"
        assert not bool((g[GUARD:GUARD + self.n] == self.poison).any()), f"{what}: an element was left unwritten"
