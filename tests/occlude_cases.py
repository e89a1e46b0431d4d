"""The cut-outs and paste cases tests/test_occlude_cpu.py derives on paper and tests/test_occlude_gpu.py compares bit for bit
(DESIGN.md section 23).  An object is (cut-out id, dst_w, dst_h, cx, cy) as datacrop.occlusion_params hands it out."""
import numpy as np

# (h, w) of the cut-outs: 5x7, 16x16, 40x23, 64x48 and a 9x12 one whose sides divide by 3
SIZES = [(5, 7), (16, 16), (40, 23), (64, 48), (9, 12)]


def cutouts():
    """uint8 RGBA with alpha 0 / 192 / 255 as the reference's masks hold (occlusion.py:81-89); cut-out 0 has every alpha value in its
    first row, whatever the draw."""
    r = np.random.default_rng(99)
    out = []
    for h, w in SIZES:
        a = r.integers(0, 256, (h, w, 4), dtype=np.uint8)
        a[..., 3] = r.choice(np.array([0, 192, 255], np.uint8), (h, w), p=[0.25, 0.25, 0.5])
        out.append(a)
    out[0][0, :3, 3] = (0, 192, 255)
    return out


def geometry(res):
    """name -> objects, for a res x res crop.  Which resize path each takes is asserted in the CPU test."""
    m = res // 2
    return {
        "none": [],
        "inside_fast_2x2": [(1, 8, 8, m, m)],                       # 16 x 16 -> 8 x 8
        "inside_copy": [(0, 7, 5, m, m)],                           # dsize == ssize, odd sizes: 7 // 2 = 3, 5 // 2 = 2
        "inside_fast_3x3": [(4, 4, 3, m, m - 1)],                   # 9 x 12 -> 3 x 4 (h x w): 3 x 3 blocks, the float product
        "inside_fast_3x4": [(3, 16, 16, m, m)],                     # 64 x 48 -> 16 x 16: blocks 4 rows x 3 columns
        "inside_mixed_axis": [(1, 8, 5, m + 1, m)],                 # x scale 2, y scale 3.2: the generic path
        "inside_generic_odd": [(2, 11, 19, m, m)],                  # 40 x 23 -> 19 x 11 (h x w)
        "inside_generic_even": [(3, 20, 26, m, m)],
        "cut_left": [(3, 20, 26, 1, m)],
        "cut_right": [(3, 20, 26, res - 1, m)],
        "cut_top": [(2, 11, 19, m, 0)],
        "cut_bottom": [(2, 11, 19, m, res)],                        # np.clip(y, 0, im_h) lets the centre sit ON the far border
        "corner": [(3, 24, 32, res, res)],                          # 2 x 2 blocks, cut by two edges
        "outside": [(1, 8, 8, -40, m)],                             # entirely outside: the crop stays untouched
        "outside_far": [(1, 8, 8, m, 10 * res)],
        "overlap_ab": [(3, 20, 26, m, m), (2, 11, 19, m + 3, m - 2)],
        "overlap_ba": [(2, 11, 19, m + 3, m - 2), (3, 20, 26, m, m)],
        "seven": [(0, 7, 5, 3, 3), (1, 8, 8, m, 4), (2, 11, 19, res - 4, m), (3, 20, 26, m - 5, m + 6), (4, 4, 3, 5, res - 2), (1, 16, 16, m, m),
                  (3, 7, 9, m + 2, m + 2)],
        # sizes whose float32 sums land on or next to x.5 for these cut-outs: a fused multiply-add in the accumulation shows here
        "near_ties_a": [(3, 32, 43, m, m)],
        "near_ties_b": [(4, 9, 7, m, m), (3, 40, 53, m, m)],
        "one_texel": [(3, 1, 1, m, m)],                             # 64 x 48 -> 1 x 1: one block over the whole cut-out
    }


PATHS = {"inside_fast_2x2": "fast", "inside_copy": "copy", "inside_fast_3x3": "fast", "inside_fast_3x4": "fast", "inside_mixed_axis": "generic",
         "inside_generic_odd": "generic", "inside_generic_even": "generic", "corner": "fast", "one_texel": "fast"}
