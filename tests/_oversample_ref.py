"""TEST INFRASTRUCTURE -- the ten-crop over-sample restated pixel by pixel on top of oracle/frames_oracle.py.

Every value is ``fixed_point_resize_pixel`` / ``resize_pixel`` evaluated at the coordinate ``(oy_k + y, ox_k + x)`` of the RESIZED frame
(a frame that already has the size is read as it is: cv::resize copies it).  The window offsets, the mirror and the 255 - v rule of the x planes
are written out here in loops; nothing is imported from tsn/frames.py (numpy slicing) or shared with csrc/vq_frames.hip.

Order and x-inversion are pyActionRecog's as remembered: PARITY UNPINNED, like the functions under test.

``fault`` injects one error, for the tests that show the comparison notices it:
"centre" (centre window one column off), "swap12" (crops 1 and 2 exchanged), "no_invert" (x plane 0 left as it is in the mirrors),
"mirror_y" (the mirror taken along y).
"""
from __future__ import annotations

import numpy as np

import frames_oracle as fo

FAULTS = ("centre", "swap12", "no_invert", "mirror_y")


def windows(h: int, w: int, crop: int, fault=None):
    """(y, x) of the five un-mirrored windows of an h x w frame: the four corners, then the centre."""
    assert crop <= h and crop <= w
    far_y, far_x = h - crop, w - crop
    five = [(0, 0), (0, far_x), (far_y, 0), (far_y, far_x), (far_y // 2, far_x // 2)]
    if fault == "centre":
        five[4] = (five[4][0], five[4][1] + (1 if five[4][1] < far_x else -1))
    if fault == "swap12":
        five[1], five[2] = five[2], five[1]
    return five


def ten_crops(img: np.ndarray, frame_size, crop: int, rule: str = "cv2", invert: bool = False, fault=None) -> np.ndarray:
    """img uint8 [H][W] or [H][W][C] -> [10][crop][crop][C] (grey: C = 1).  ``invert``: the mirrored crops store 255 - v."""
    out_w, out_h = frame_size
    rows = img.tolist()
    grey = img.ndim == 2
    channels = 1 if grey else img.shape[2]
    same = img.shape[:2] == (out_h, out_w)
    pixel = {"cv2": fo.fixed_point_resize_pixel, "exact": fo.resize_pixel}[rule]
    seen = {}

    def value(ry, rx, ch):
        key = (ry, rx, ch)
        if key not in seen:
            if same:
                seen[key] = rows[ry][rx] if grey else rows[ry][rx][ch]
            else:
                seen[key] = pixel(rows, ry, rx, out_h, out_w, None if grey else ch)
        return seen[key]

    out = np.zeros((10, crop, crop, channels), dtype=np.uint8)
    for k, (oy, ox) in enumerate(windows(out_h, out_w, crop, fault)):
        for y in range(crop):
            for x in range(crop):
                for ch in range(channels):
                    v = value(oy + y, ox + x, ch)
                    out[k][y][x][ch] = v
                    m = 255 - v if invert else v
                    if fault == "mirror_y":
                        out[5 + k][crop - 1 - y][x][ch] = m
                    else:
                        out[5 + k][y][crop - 1 - x][ch] = m
    return out


def ten_crops_flow_stack(planes, frame_size, crop: int, rule: str = "cv2", fault=None) -> np.ndarray:
    """[x0, y0, x1, y1, ...] grey frames of one snippet -> [10][crop][crop][len(planes)]; the x planes (even) inverted in the mirrors."""
    out = np.zeros((10, crop, crop, len(planes)), dtype=np.uint8)
    for p, plane in enumerate(planes):
        invert = p % 2 == 0 and not (fault == "no_invert" and p == 0)
        one = ten_crops(plane, frame_size, crop, rule, invert, fault)
        for k in range(10):
            for y in range(crop):
                for x in range(crop):
                    out[k][y][x][p] = one[k][y][x][0]
    return out
