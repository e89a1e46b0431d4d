"""The shapes and settings tests/test_datacrop_gpu.py compares bit for bit (and tests/test_datacrop_cpu.py checks for coverage):
two images of different sizes, every rotation x scale x flip x noise combination, and boxes inside, across each border, outside,
larger than the image, with half-integer centres, and image indices outside the table."""
import itertools

import numpy as np

ROTS = [0.0, 30.0, -47.5, 90.0, 180.0]
SCS = [0.75, 1.0, 1.25]
FLIPS = [0, 1]
PNS = [(1.0, 1.0, 1.0), (0.6, 1.4, 1.0)]                  # 1.4 forces the clamp at 255
# (image, centre x, centre y, scale = box side / 200): image 0 is 61 x 83 (H x W), image 1 is 270 x 480
BOXES = [(0, 40.0, 30.0, 0.2),            # fully inside
         (1, 240.0, 135.0, 0.9),          # inside the larger image
         (0, 2.0, 30.0, 0.2),             # across the left border
         (0, 81.0, 30.0, 0.2),            # right
         (0, 40.0, 1.0, 0.2),             # top
         (0, 40.0, 59.0, 0.2),            # bottom
         (0, -200.0, -200.0, 0.2),        # fully outside: all zero
         (0, 41.0, 30.0, 1.0),            # larger than the image
         (1, 0.5, 1.5, 0.3),              # half-integer centres: round half to even gives (0, 2)
         (0, 40.5, 21.5, 0.155),          # (40, 22); box side 31
         (7, 30.0, 30.0, 0.2),            # image index past the table: clamped to the last image
         (-3, 30.0, 30.0, 0.2),           # negative index: clamped to the first
         (1, 478.0, 268.0, 0.25)]         # the bottom-right corner of the larger image


def images():
    r = np.random.default_rng(2024)
    return [r.integers(0, 256, (61, 83, 3), dtype=np.uint8), r.integers(0, 256, (270, 480, 3), dtype=np.uint8)]


def catalogue():
    """Every (rot, sc, flip, pn) combination once, the boxes cycling under them with a stride that mixes both: 60 settings, then
    every box once more at the identity.  Rows: dict(img, center, scale, rot, sc, flip, pn)."""
    rows = []
    for k, (rot, sc, flip, pn) in enumerate(itertools.product(ROTS, SCS, FLIPS, PNS)):
        b = BOXES[(5 * k + k // len(BOXES)) % len(BOXES)]
        rows.append(dict(img=b[0], center=(b[1], b[2]), scale=b[3], rot=rot, sc=sc, flip=flip, pn=pn))
    for b in BOXES:
        rows.append(dict(img=b[0], center=(b[1], b[2]), scale=b[3], rot=0.0, sc=1.0, flip=0, pn=PNS[0]))
    # a prefix of any length >= 5 should already see a rotation, a flip, a clamp and a border: deal the rows out with a stride
    order = [(17 * i) % len(rows) for i in range(len(rows))]
    assert sorted(order) == list(range(len(rows)))
    return [rows[i] for i in order]


def columns(rows):
    return dict(img=[r["img"] for r in rows], center=[r["center"] for r in rows], scale=[r["scale"] for r in rows],
                rot=[r["rot"] for r in rows], sc=[r["sc"] for r in rows], flip=[r["flip"] for r in rows], pn=[r["pn"] for r in rows])
