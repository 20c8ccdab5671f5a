"""What the tests that compile the host planner on its own share: its source
list, and the input lines of tests/native/plan_driver.cpp."""
import json
import os

from flyimg_amd import _lib as L
from flyimg_amd.processor import ExecFailedException, ImageProcessor, OptionsBag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the host-only planner (everything fi_plan.h declares), linkable without HIP
PLANNER_SRCS = [os.path.join(ROOT, "flyimg_amd/csrc", f) for f in ("fi_plan.cpp", "fi_plan_mfma.cpp", "fi_plan_sc.cpp")]


def plan_lines():
    """(W, H, C, target_w, target_h, flags, gravity, rotate, smartcrop_w, smartcrop_h) per image"""
    lines = []
    with open(os.path.join(ROOT, "tests/golden/im_geometry_cases.json")) as f:
        cases = json.load(f)
    for c in cases:
        C = 4 if c.get("mode") == "RGBA" else 3
        try:
            op = ImageProcessor(OptionsBag(c["options"]), c["src_w"], c["src_h"]).to_op()
        except ExecFailedException:
            continue
        lines.append((c["src_w"], c["src_h"], C, op.target_w, op.target_h, op.flags, op.gravity, op.rotate, 0, 0))
    with open(os.path.join(ROOT, "tests/golden/smartcrop_golden.json")) as f:
        sc = json.load(f)
    for c in sc["cases"]:
        lines.append((c["w"], c["h"], 3, 0, 0, L.FI_OP_THUMBNAIL | L.FI_OP_SMARTCROP, 5, 0, 100, 100))
    T, F, S, E, G, R = (L.FI_OP_THUMBNAIL, L.FI_GEOM_FILL, L.FI_GEOM_SHRINK_ONLY, L.FI_OP_EXTENT, L.FI_OP_GRAY,
                        L.FI_OP_ROTATE)
    edge = [
        (1, 1, 3, 1, 1, T, 5, 0), (2, 1, 3, 1, 1, T | F | E, 5, 0), (1, 5000, 3, 1, 0, T, 5, 0),
        (5000, 1, 3, 0, 1, T, 5, 0), (6000, 4000, 3, 400, 400, T | F | E | G | R, 5, 90),
        (3840, 2160, 3, 512, 512, T | F | E, 1, 0), (1920, 1080, 3, 500, 0, T | S, 5, 0),
        (120, 90, 3, 4000, 0, T, 5, 0), (640, 481, 3, 317, 0, L.FI_OP_RESIZE | S, 5, 0),
        (900, 600, 4, 250, 300, L.FI_OP_RESIZE | F | E | R, 9, 270), (800, 600, 3, 200, 0, T | L.FI_OP_MONOCHROME, 5, 0),
        (333, 222, 3, 200, 0, T | S | R | L.FI_SRC_PSEUDOCLASS, 5, 180), (16, 16, 3, 16, 16, T, 5, 0),
        (5657, 4243, 3, 300, 250, T | F | E, 5, 0), (530, 942, 3, 0, 300, T, 5, 0),
    ]
    for e in edge:
        lines.append(e + (0, 0))
        lines.append(e[:5] + (e[5] | L.FI_OP_SMARTCROP,) + e[6:] + (100, 56))
    # every table variant of the planner (the driver's DONE line counts them)
    SC, RS = L.FI_OP_SMARTCROP, L.FI_OP_RESIZE
    lines += [
        # the BASELINE geometries: cfg1's uneven touched rows (ThumbnailImage's sample pre-step) and cfg5
        (3000, 2000, 3, 300, 250, T | F | E, 5, 0, 0, 0), (6000, 4000, 3, 400, 400, T | F | E, 5, 0, 0, 0),
        # slight and strong -resize reductions: one and two k-steps per 16-output block on both axes
        (1000, 700, 3, 333, 0, RS | S, 5, 0, 0, 0), (2000, 1500, 3, 500, 0, RS | S, 5, 0, 0, 0),
        (1001, 3000, 3, 333, 0, T | S, 5, 0, 0, 0),  # horizontal first
        # smartcrop with no resample before it, so the prescale alone sets the factor: Pillow's
        # reduce (6000x4000), a factor between 3 and 4 (two k-steps, windows past k_sc_vq's 64 rows),
        # a factor below 2 (one k-step), and a window narrower than 64 columns
        (6000, 4000, 3, 0, 0, SC, 5, 0, 100, 100), (400, 390, 3, 0, 0, SC, 5, 0, 100, 100),
        (250, 180, 3, 0, 0, SC, 5, 0, 100, 100), (640, 480, 3, 0, 0, SC, 5, 0, 40, 30),
        (1920, 1080, 3, 0, 0, SC | G, 5, 0, 100, 100),
        (800, 600, 3, 200, 0, T | R | L.FI_OP_ROTATE_SHEAR | L.FI_OP_BACKGROUND, 5, 17, 0, 0),  # ShearPlan
    ]
    return lines
